// spt_noise.h — one pixel of the noise estimate (include/spt.h "noise estimate"): the batch-moment update, the
// squared relative error of a pixel and its bin. The single source of the device kernels (spt_noise.hip) and of
// the host entry points (spt_noise_update_host, spt_noise_meter_host): integer operations, comparisons and
// `+ - * /` in fp32, compiled without contraction on both sides, so both give the same bits. Internal.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

#include "spt.h"

namespace spt {

// The key (float bits >> 20) of bin 0: 2^-28, a relative error of 0.006 %. 256 bins of an eighth of an octave
// reach 2^4 from there, a relative error of 400 %: the range a progressive render crosses from its second batch
// to long after it stopped changing visibly (spt.h). Moving it moves every histogram: not without a reason.
constexpr int kNoiseKeyBase = 792;
constexpr int kNoiseMaxRadius = 2;

// What a batch of w frames folds with, computed once per update on the host: w, the frames folded with it
// (Wn = W + w) and r = w / Wn.
struct NoiseBatch {
    float w, r;
};

// The luminance of an accumulation's pixel (the sums, not the mean: a batch is a difference of two).
__host__ __device__ inline float noise_luminance(float4 a) { return (0.2126f * a.x + 0.7152f * a.y) + 0.0722f * a.z; }

// One pixel's state (mean, m2, prevL, 0) after the batch that brought its accumulation to a.
__host__ __device__ inline float4 noise_update_pixel(float4 a, float4 s, NoiseBatch b) {
    const float L = noise_luminance(a);
    const float d = (L - s.z) / b.w;
    const float delta = d - s.x;
    const float mean = s.x + b.r * delta;
    const float m2 = s.y + (b.w * delta) * (d - mean);
    return make_float4(mean, m2, L, 0.0f);
}

// The squared relative standard error of the mean luminance from a pixel's (pooled) moments;
// inv = 1 / ((B - 1) * W).
__host__ __device__ inline float noise_e2(float s_mean, float s_m2, float inv, float dark_floor) {
    const float v = s_m2 * inv;
    const float t = s_mean + dark_floor;
    return v / (t * t);
}

__host__ __device__ inline uint32_t noise_bin(float e2) {
    if (e2 != e2) return SPT_NOISE_BINS - 1;
    if (!(e2 > 0.0f)) return 0u;
    uint32_t bits;
    __builtin_memcpy(&bits, &e2, sizeof(bits));
    const int key = (int)(bits >> 20);
    const int b = (key < kNoiseKeyBase ? kNoiseKeyBase : key) - kNoiseKeyBase;
    return (uint32_t)(b < SPT_NOISE_BINS - 1 ? b : SPT_NOISE_BINS - 1);
}

// The taps of pixel (x, y)'s window that lie inside a width x height image, as a float.
__host__ __device__ inline float noise_tap_count(int x, int y, int width, int height, int radius) {
    const int x0 = x - radius < 0 ? 0 : x - radius, x1 = x + radius > width - 1 ? width - 1 : x + radius;
    const int y0 = y - radius < 0 ? 0 : y - radius, y1 = y + radius > height - 1 ? height - 1 : y + radius;
    return (float)((x1 - x0 + 1) * (y1 - y0 + 1));
}

// Pixel (x, y)'s e2 with its window pooled (radius 1 or 2), the taps read through tap(tx, ty) -> (mean, m2) for
// taps inside the image only, rows outer, columns inner, each sum started at 0.0f.
template <class Tap>
__host__ __device__ inline float noise_pooled_e2(int x, int y, int width, int height, int radius, float inv,
                                                 float dark_floor, Tap tap) {
    float s_mean = 0.0f, s_m2 = 0.0f;
    for (int ty = y - radius; ty <= y + radius; ++ty) {
        if (ty < 0 || ty >= height) continue;
        for (int tx = x - radius; tx <= x + radius; ++tx) {
            if (tx < 0 || tx >= width) continue;
            const float2 t = tap(tx, ty);
            s_mean = s_mean + t.x;
            s_m2 = s_m2 + t.y;
        }
    }
    const float n = noise_tap_count(x, y, width, height, radius);
    return noise_e2(s_mean / n, s_m2 / n, inv, dark_floor);
}

// ---- the definition's host part, shared by spt_capi_post.hip and spt_host.cpp (the parameters': spt_params.h) ----
constexpr float kNoiseMaxFrames = 16777216.0f;  // 2^24: W stays an exact integer in a float

// a frame count held in a float: an integer in [1, 2^24]
inline bool noise_count_ok(float frames) {
    return frames >= 1.0f && frames <= kNoiseMaxFrames && frames == (float)(uint32_t)frames;
}
// an update's: a batch of w frames onto W
inline NoiseBatch noise_batch(float w, float W) { return NoiseBatch{w, w / (W + w)}; }
// a metering's
inline float noise_inv(uint32_t batches, float W) { return 1.0f / ((float)(batches - 1u) * W); }
// nullptr: a valid image, B and W
inline const char* noise_image_error(uint32_t width, uint32_t height, uint32_t batches, float frames) {
    if (width == 0 || height == 0 || (uint64_t)width * height >= (1ull << 31)) return "noise meter: an empty or too large image";
    if (batches < 2) return "noise meter: fewer than two batches";
    if (!noise_count_ok(frames)) return "noise meter: frames must be an integer in [1, 2^24]";
    return nullptr;
}

// state[i] = noise_update_pixel(accum[i], state[i], b) for i in [0, n)
void launch_noise_update(const float4* accum, float4* state, uint64_t n, NoiseBatch b, hipStream_t s);
// counts[0..255] += the histogram of the e2 of a width x height image of moments (the caller zeroes them on the
// stream first); e2 (may be nullptr): the per-pixel values. radius 0..2.
void launch_noise_meter(const float4* state, uint32_t width, uint32_t height, int radius, float inv, float dark_floor,
                        uint32_t* counts, float* e2, hipStream_t s);

}  // namespace spt
