// spt_atrous_guided.h — one pixel of the variance-guided a-trous filter (include/spt.h "variance-guided
// denoiser"): the variance of the mean luminance from the noise moments, its 3 x 3 prefilter, and one level of
// the filter with the variance it propagates. The single source of the device kernels (spt_denoise_guided.hip)
// and of spt_atrous_guided_host: `+ - * /` and fmaxf in fp32, compiled without contraction on both sides, so
// both give the same bits. Internal.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

#include "spt.h"
#include "spt_atrous.h"

namespace spt {

// What a level reads of one pixel: the colour with its linear luminance, the first hit's position and
// material, its shading normal, and the variance of its luminance.
struct GuidedTap {
    float r, g, b, lum;
    float px, py, pz;
    uint32_t mat;
    float nx, ny, nz;
    float var;
};

// The constants of level l (step 1 << l), computed once on the host for the device and the host filter.
struct GuidedLevel {
    int step;
    float s2, floor, inv_z;  // sigma_variance^2, variance_floor, 1 / (sigma_plane * step)
    uint32_t normal_power_log2;
};
inline GuidedLevel guided_level(uint32_t l, const spt_guided_params& p) {
    const int s = 1 << l;
    return GuidedLevel{s, p.sigma_variance * p.sigma_variance, p.variance_floor, 1.0f / (p.sigma_plane * (float)s),
                       p.normal_power_log2};
}
// inv = 1 / ((B - 1) * frame_count): m2 * inv is the variance of the mean of frame_count frames
inline float guided_inv(uint32_t batches, uint32_t frame_count) {
    return 1.0f / ((float)(batches - 1u) * (float)frame_count);
}

// linear: the variance is the linear luminance's
__host__ __device__ inline float guided_lum(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }

__host__ __device__ inline GuidedTap guided_tap(float4 c, float4 fa, float4 fb, float var) {
    uint32_t mat;
    __builtin_memcpy(&mat, &fa.w, sizeof(mat));
    return GuidedTap{c.x, c.y, c.z, guided_lum(c.x, c.y, c.z), fa.x, fa.y, fa.z, mat, fb.x, fb.y, fb.z, var};
}

// v0 of a pixel's moments (mean, m2, prevL, 0)
__host__ __device__ inline float guided_variance0(float m2, float inv) { return fmaxf(m2 * inv, 0.0f); }

// The prefiltered variance of pixel (x, y). v0(qx, qy): asked for taps inside the image only.
template <class Fetch>
__host__ __device__ inline float guided_prefilter_pixel(int x, int y, int w, int h, Fetch&& v0) {
    const float G[3] = {0.25f, 0.5f, 0.25f};
    float s = 0.0f, sg = 0.0f;
    for (int j = 0; j < 3; ++j) {
        const int qy = y + j - 1;
        for (int i = 0; i < 3; ++i) {
            const int qx = x + i - 1;
            if (qx < 0 || qy < 0 || qx >= w || qy >= h) continue;
            const float g = G[j] * G[i];
            s = s + g * v0(qx, qy);
            sg = sg + g;
        }
    }
    return s / sg;
}

// The filtered colour of pixel (x, y), whose own record is `p` and whose alpha is `alpha`, and in *out_v the
// variance it propagates. fetch(i, j, qx, qy): the record of tap (i, j) at pixel (qx, qy), asked for taps
// inside the image only.
template <class Fetch>
__host__ __device__ inline float4 guided_pixel(const GuidedTap& p, float alpha, int x, int y, int w, int h,
                                               const GuidedLevel& lv, Fetch&& fetch, float* out_v) {
    if (p.mat == kFeatMiss) {  // the sky passes through, its variance too
        *out_v = p.var;
        return make_float4(p.r, p.g, p.b, alpha);
    }
    const float H[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
    const float iv = 1.0f / (lv.s2 * p.var + lv.floor);
    float sr = 0.0f, sg = 0.0f, sb = 0.0f, sw = 0.0f, sv = 0.0f;
    for (int j = 0; j < 5; ++j) {
        const int qy = y + (j - 2) * lv.step;
        for (int i = 0; i < 5; ++i) {
            const int qx = x + (i - 2) * lv.step;
            if (qx < 0 || qy < 0 || qx >= w || qy >= h) continue;
            const GuidedTap q = fetch(i, j, qx, qy);
            const float dl = q.lum - p.lum;
            const float x2 = (dl * dl) * iv;
            const float r = 1.0f / (1.0f + x2);
            const float wc = (H[j] * H[i]) * (r * r);
            float dn = fmaxf((p.nx * q.nx + p.ny * q.ny) + p.nz * q.nz, 0.0f);
            for (uint32_t n = 0; n < lv.normal_power_log2; ++n) dn = dn * dn;
            const float ex = q.px - p.px, ey = q.py - p.py, ez = q.pz - p.pz;
            const float pd = ((p.nx * ex + p.ny * ey) + p.nz * ez) * lv.inv_z;
            const float rz = 1.0f / (1.0f + pd * pd);
            const float geo = dn * (rz * rz);
            float wt = wc * geo;
            if (q.mat != p.mat) wt = 0.0f;
            sr = sr + wt * q.r;
            sg = sg + wt * q.g;
            sb = sb + wt * q.b;
            sw = sw + wt;
            sv = sv + (wt * wt) * q.var;
        }
    }
    *out_v = sv / (sw * sw);
    return make_float4(sr / sw, sg / sw, sb / sw, alpha);
}

}  // namespace spt
