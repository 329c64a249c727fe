// spt_reproject.h — temporal reprojection (include/spt.h "temporal reprojection"): one pixel of the gather
// that maps a captured view into the current one, and one pixel of the blend of that history with the
// frames accumulated since. The single source of the device kernels (spt_reproject.hip) and of
// spt_reproject_host: `+ - * /`, floorf, fabsf, fminf and comparisons in fp32, compiled without contraction
// on both sides, so both give the same bits. Also the kernels' host launchers. Internal.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

#include "spt.h"
#include "spt_atrous.h"

namespace spt {

// The captured view's camera as the gather reads it: the dual basis of (u, v, w), its origin and the
// offset of its features' rays inside their pixels. Passed to the kernel by value.
struct ReprojectView {
    float ru[3], rv[3], rw[3];
    float o[3];
    float j;
};

// In double from the camera's float fields, rounded once; all rows zero for a vanishing or non-finite
// determinant (nothing is reused then). nullptr: the reference's camera.
inline ReprojectView reproject_view(const spt_camera* cam) {
    ReprojectView r{{1.f, 0.f, 0.f}, {0.f, 1.f, 0.f}, {0.f, 0.f, 1.f}, {0.f, 0.f, 0.f}, 0.f};
    if (!cam) return r;
    auto cross = [](const double a[3], const double b[3], double out[3]) {
        out[0] = a[1] * b[2] - a[2] * b[1];
        out[1] = a[2] * b[0] - a[0] * b[2];
        out[2] = a[0] * b[1] - a[1] * b[0];
    };
    const double u[3] = {cam->u[0], cam->u[1], cam->u[2]}, v[3] = {cam->v[0], cam->v[1], cam->v[2]},
                 w[3] = {cam->w[0], cam->w[1], cam->w[2]};
    double vw[3], wu[3], uv[3];
    cross(v, w, vw);
    cross(w, u, wu);
    cross(u, v, uv);
    const double det = (u[0] * vw[0] + u[1] * vw[1]) + u[2] * vw[2];
    const bool ok = det != 0.0 && std::isfinite(det);
    for (int a = 0; a < 3; ++a) {
        r.ru[a] = ok ? (float)(vw[a] / det) : 0.0f;
        r.rv[a] = ok ? (float)(wu[a] / det) : 0.0f;
        r.rw[a] = ok ? (float)(uv[a] / det) : 0.0f;
        r.o[a] = cam->origin[a];
    }
    r.j = (cam->flags & SPT_CAMERA_JITTER) ? 0.5f : 0.0f;
    return r;
}

// The history of the pixel whose current features are (fa, fb), gathered from the captured view's w x h
// images: (mean radiance, length in frames), or zeros where nothing is reused. reusable: one word per
// material, 0 where its radiance depends on the eye (nullptr: every material is reusable).
// tap_a(q) / tap_b(q) / tap_c(q): the captured feat_a / feat_b / image at pixel index q, asked for taps
// inside the image only, in that order, the image for a valid tap only.
template <class TapA, class TapB, class TapC>
__host__ __device__ inline float4 reproject_pixel(float4 fa, float4 fb, int w, int h, const ReprojectView& v,
                                                  const spt_reproject_params& p, const uint32_t* reusable,
                                                  uint32_t n_materials, TapA&& tap_a, TapB&& tap_b, TapC&& tap_c) {
    const float4 none = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    uint32_t mat;
    __builtin_memcpy(&mat, &fa.w, sizeof(mat));
    if (mat == kFeatMiss) return none;
    if (reusable && (mat >= n_materials || reusable[mat] == 0u)) return none;
    const float ex = fa.x - v.o[0], ey = fa.y - v.o[1], ez = fa.z - v.o[2];
    const float a = (v.ru[0] * ex + v.ru[1] * ey) + v.ru[2] * ez;
    const float b = (v.rv[0] * ex + v.rv[1] * ey) + v.rv[2] * ez;
    const float c = (v.rw[0] * ex + v.rw[1] * ey) + v.rw[2] * ez;
    if (!(c > 0.0f)) return none;
    const float Wf = (float)w, Hf = (float)h;
    const float aspect = Wf / Hf;
    const float sx = a / c, sy = b / c;
    const float fx = ((sx / aspect + 1.0f) * 0.5f) * Wf - v.j;
    const float fy = (1.0f - (sy + 1.0f) * 0.5f) * Hf - v.j;
    if (!(fx > -1.0f && fx < Wf && fy > -1.0f && fy < Hf)) return none;  // (NaN and inf too)
    const float x0f = floorf(fx), y0f = floorf(fy);
    const float ax = fx - x0f, ay = fy - y0f;
    const int x0 = (int)x0f, y0 = (int)y0f;  // in [-1, w - 1] x [-1, h - 1]
    const float bound = p.plane_tolerance * fb.w;
    float sr = 0.0f, sg = 0.0f, sb = 0.0f, sn = 0.0f, sw = 0.0f;
    for (int j = 0; j < 2; ++j) {
        const int qy = y0 + j;
        for (int i = 0; i < 2; ++i) {
            const int qx = x0 + i;
            if (qx < 0 || qy < 0 || qx >= w || qy >= h) continue;
            const size_t q = (size_t)qy * (size_t)w + (size_t)qx;
            const float4 ha = tap_a(q);
            uint32_t qmat;
            __builtin_memcpy(&qmat, &ha.w, sizeof(qmat));
            if (qmat != mat) continue;
            const float4 hb = tap_b(q);
            if (!((fb.x * hb.x + fb.y * hb.y) + fb.z * hb.z >= p.normal_min)) continue;
            const float dx = ha.x - fa.x, dy = ha.y - fa.y, dz = ha.z - fa.z;
            if (!(fabsf((fb.x * dx + fb.y * dy) + fb.z * dz) <= bound)) continue;
            const float k = (i ? ax : 1.0f - ax) * (j ? ay : 1.0f - ay);
            const float4 hc = tap_c(q);
            sr = sr + k * hc.x;
            sg = sg + k * hc.y;
            sb = sb + k * hc.z;
            sn = sn + k * hc.w;
            sw = sw + k;
        }
    }
    if (!(sw >= p.min_weight)) return none;
    return make_float4(sr / sw, sg / sw, sb / sw, fminf(sn / sw, p.max_history));
}

// The history h (zeros: none) combined with the sums `acc` of the f frames accumulated since. kLength:
// alpha is the result's length in frames (what a capture stores), else the mean's own alpha (what is shown).
template <bool kLength>
__host__ __device__ inline float4 history_blend_pixel(float4 acc, float f, float4 h) {
    const float4 m = make_float4(acc.x / f, acc.y / f, acc.z / f, acc.w / f);
    float4 out = m;
    if (h.w > 0.0f) {
        const float n = h.w + f;
        out.x = (h.x * h.w + m.x * f) / n;
        out.y = (h.y * h.w + m.y * f) / n;
        out.z = (h.z * h.w + m.z * f) / n;
    }
    out.w = kLength ? h.w + f : m.w;
    return out;
}

// The two layouts of a captured view in its 3 * pixels float4, same bits:
// planes: the image, feat_a and feat_b one after the other; records: (feat_a, feat_b, image) per pixel, 48 B.
constexpr int kHistoryPlanes = 0;
constexpr int kHistoryRecords = 1;
constexpr int kHistoryDefault = kHistoryPlanes;  // measured: profiles/reproject_rates.txt

// view[...] = the capture of (accum / frames blended with hist, or alone for hist == nullptr) and the features
void launch_history_capture(int layout, const float4* accum, float frames, const float4* hist, const float4* feat_a,
                            const float4* feat_b, float4* view, uint32_t pixels, hipStream_t s);
// out = that blend with the mean's alpha
void launch_history_blend(const float4* accum, float frames, const float4* hist, float4* out, uint32_t pixels,
                          hipStream_t s);
// out = the captured view (in `layout`) gathered into the view of the current features
void launch_reproject(int layout, const float4* feat_a, const float4* feat_b, const float4* view, float4* out, uint32_t w,
                      uint32_t h, const ReprojectView& v, const spt_reproject_params& p, const uint32_t* reusable,
                      uint32_t n_materials, hipStream_t s);

}  // namespace spt
