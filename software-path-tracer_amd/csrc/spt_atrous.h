// spt_atrous.h — one pixel of one level of the edge-avoiding a-trous filter (include/spt.h "denoiser"),
// the single source of the device kernels (spt_denoise.hip) and of spt_atrous_host: `+ - * /` and fmaxf
// in fp32, compiled without contraction on both sides, so both give the same bits. Internal.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace spt {

constexpr uint32_t kFeatMiss = 0xffffffffu;  // feat_a.w of a pixel whose camera ray missed
constexpr uint32_t kAtrousMaxLevels = 6;
constexpr uint32_t kAtrousMaxNormalPower = 7;

// What a level reads of one pixel: the mean colour with its compressed luminance, the first hit's
// position and material, and its shading normal.
struct AtrousTap {
    float r, g, b, lum;
    float px, py, pz;
    uint32_t mat;
    float nx, ny, nz;
};

// The constants of level l (step 1 << l), computed once on the host for the device and the host filter.
struct AtrousLevel {
    int step;
    float inv_c, inv_z;
    uint32_t normal_power_log2;
};
inline AtrousLevel atrous_level(uint32_t l, float sigma_color, float sigma_plane, uint32_t normal_power_log2) {
    const int s = 1 << l;
    return AtrousLevel{s, 1.0f / (sigma_color * (1.0f / (float)s)), 1.0f / (sigma_plane * (float)s), normal_power_log2};
}

// lum(v) = L / (1 + L): compressed, so that a firefly is an outlier among its neighbours at any value
__host__ __device__ inline float atrous_lum(float r, float g, float b) {
    const float L = (0.2126f * r + 0.7152f * g) + 0.0722f * b;
    return L / (1.0f + L);
}

__host__ __device__ inline AtrousTap atrous_tap(float4 c, float4 fa, float4 fb) {
    uint32_t mat;
    __builtin_memcpy(&mat, &fa.w, sizeof(mat));
    return AtrousTap{c.x, c.y, c.z, atrous_lum(c.x, c.y, c.z), fa.x, fa.y, fa.z, mat, fb.x, fb.y, fb.z};
}

// The filtered colour of pixel (x, y), whose own record is `p` and whose alpha is `alpha`.
// fetch(i, j, qx, qy): the record of tap (i, j) at pixel (qx, qy), asked for taps inside the image only.
template <class Fetch>
__host__ __device__ inline float4 atrous_pixel(const AtrousTap& p, float alpha, int x, int y, int w, int h,
                                               const AtrousLevel& lv, Fetch&& fetch) {
    if (p.mat == kFeatMiss) return make_float4(p.r, p.g, p.b, alpha);  // the sky passes through
    const float H[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
    float sr = 0.0f, sg = 0.0f, sb = 0.0f, sw = 0.0f;
    for (int j = 0; j < 5; ++j) {
        const int qy = y + (j - 2) * lv.step;
        for (int i = 0; i < 5; ++i) {
            const int qx = x + (i - 2) * lv.step;
            if (qx < 0 || qy < 0 || qx >= w || qy >= h) continue;
            const AtrousTap q = fetch(i, j, qx, qy);
            const float k = H[j] * H[i];
            const float dl = (q.lum - p.lum) * lv.inv_c;
            const float r = 1.0f / (1.0f + dl * dl);
            const float wc = k * (r * r);
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
        }
    }
    return make_float4(sr / sw, sg / sw, sb / sw, alpha);
}

}  // namespace spt
