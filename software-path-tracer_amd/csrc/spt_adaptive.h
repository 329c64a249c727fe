// spt_adaptive.h — the definition of adaptive sampling's per-pixel steps, ahead of the kernels that will run them:
// the window vote of a round's selection, and the mean and the resolve of an accumulation whose pixels hold
// different frame counts (.w). `__host__ __device__` functions in the style of spt_noise.h: integer operations,
// comparisons and `* /` in fp32, compiled without contraction, so a host build and a device build give the same
// bits. Nothing in the library includes this header yet; tests/test_adaptive_host.py pins it, through
// tests/cpp/adaptive_host_check.cpp, to the numpy restatement in tests/adaptive_ref.py. Internal.
//
// State per pixel p of a width x height image: stop[p] (uint32), 0 while the pixel is active, otherwise the frame
// count at which it retired; e2[p], the noise estimate's squared relative error at the pixel's last fold
// (spt_noise.h noise_e2). One selection, after B batches of F frames in all: active pixel p keeps tracing if
// B < min_batches, or if some pixel q of p's (2 * radius + 1)^2 window inside the image (rows outer, columns
// inner, p among them) has stop[q] == 0 and !(e2[q] <= rel_error * rel_error) — so a NaN keeps its neighbours
// active. Every other active pixel retires (the caller sets stop[p] = F). A retired pixel never comes back.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

#include "spt_display.h"

namespace spt {

constexpr int kAdaptiveMaxRadius = 2;

struct AdaptiveParams {
    float rel_error;       // a pixel may retire once its relative standard error is <= this; > 0, finite
    uint32_t radius;       // 0..2: the window of the vote
    uint32_t min_batches;  // nothing retires before this many batches are folded; >= 2
};
constexpr AdaptiveParams kAdaptiveDefaults = {0.02f, 1u, 4u};

// nullptr: valid
inline const char* adaptive_params_error(const AdaptiveParams& p) {
    if (!(p.rel_error > 0.0f) || !std::isfinite(p.rel_error)) return "adaptive: rel_error must be > 0 and finite";
    if (p.radius > (uint32_t)kAdaptiveMaxRadius) return "adaptive: radius must be 0, 1 or 2";
    if (p.min_batches < 2u) return "adaptive: min_batches must be >= 2";
    return nullptr;
}
// the target the votes compare e2 with: the square in fp32, once
inline float adaptive_target(const AdaptiveParams& p) { return p.rel_error * p.rel_error; }

// Whether pixel q keeps its neighbours tracing: it is active and not at the target (`!(e2 <= t2)`: a NaN votes).
__host__ __device__ inline bool adaptive_votes(uint32_t stop, float e2, float t2) { return stop == 0u && !(e2 <= t2); }

// Whether active pixel (x, y) keeps tracing: some tap of its window inside the image votes; taps read through
// votes(tx, ty) -> bool, rows outer, columns inner, the pixel itself among them.
template <class Tap>
__host__ __device__ inline bool adaptive_keep(int x, int y, int width, int height, int radius, Tap votes) {
    for (int ty = y - radius; ty <= y + radius; ++ty) {
        if (ty < 0 || ty >= height) continue;
        for (int tx = x - radius; tx <= x + radius; ++tx) {
            if (tx < 0 || tx >= width) continue;
            if (votes(tx, ty)) return true;
        }
    }
    return false;
}

// One pixel of the mean image: the sums over the pixel's own frame count, which stays in .w; no frames, all zero.
__host__ __device__ inline float4 adaptive_mean_pixel(float4 a) {
    if (a.w == 0.0f) return make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    return make_float4(a.x / a.w, a.y / a.w, a.z / a.w, a.w);
}

// One pixel's RGBA8: k_resolve's expression (spt_kernels.hip rgba8) with the pixel's own a.w as the frame count
__host__ __device__ inline uint32_t adaptive_rgba8(float4 a, float exposure) {
    const float f = a.w;
    return (display_u8((a.x / f) * exposure) << 24) | (display_u8((a.y / f) * exposure) << 16) |
           (display_u8((a.z / f) * exposure) << 8) | display_u8(a.w / f);
}

// One selection over an image on the host: keep[p] = 1 for an active pixel that keeps tracing, 0 for one that
// retires and for a retired one. false: invalid parameters, an empty image, or batches or frames of 0.
inline bool adaptive_select_image(const float* e2, const uint32_t* stop, uint32_t width, uint32_t height, uint32_t batches,
                                  uint32_t frames, const AdaptiveParams& p, uint8_t* keep) {
    if (!e2 || !stop || !keep || adaptive_params_error(p)) return false;
    if (width == 0 || height == 0 || (uint64_t)width * height >= (1ull << 31)) return false;
    if (batches < 1u || frames < 1u || frames > (1u << 24)) return false;
    const float t2 = adaptive_target(p);
    const bool keep_all = batches < p.min_batches;
    const int w = (int)width, h = (int)height, radius = (int)p.radius;
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            const size_t i = (size_t)y * width + x;
            bool k = false;
            if (stop[i] == 0u)
                k = keep_all || adaptive_keep(x, y, w, h, radius, [&](int tx, int ty) {
                        const size_t q = (size_t)ty * width + tx;
                        return adaptive_votes(stop[q], e2[q], t2);
                    });
            keep[i] = k ? 1u : 0u;
        }
    return true;
}

}  // namespace spt
