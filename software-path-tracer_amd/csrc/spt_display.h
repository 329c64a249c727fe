// spt_display.h — one pixel of the luminance meter and of the display transform (include/spt.h "exposure and
// tone mapping"), the single source of the device kernels (spt_display.hip) and of the host entry points
// (spt_meter_bin, spt_luminance_histogram_host, spt_display_host): integer operations, comparisons and
// `* + /` in fp32, compiled without contraction on both sides, so both give the same bits. Internal.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "spt.h"

namespace spt {

constexpr int kMeterKeyBase = 888;  // the key (float bits >> 20) of bin 0's upper end: 2^-16 * 1.125 starts bin 1

// The bin of luminance L: its exponent and three mantissa bits, from 2^-16 up. NaN, zero and negatives: bin 0.
__host__ __device__ inline uint32_t meter_bin(float L) {
    uint32_t bits;
    __builtin_memcpy(&bits, &L, sizeof(bits));
    const int key = L > 0.0f ? (int)(bits >> 20) : 0;
    const int b = (key < kMeterKeyBase ? kMeterKeyBase : key) - kMeterKeyBase;
    return (uint32_t)(b < SPT_METER_BINS - 1 ? b : SPT_METER_BINS - 1);
}

// The denoiser's luminance (spt_atrous.h atrous_lum before its compression) of p / divisor.
__host__ __device__ inline float pixel_luminance(float4 p, float divisor) {
    const float r = p.x / divisor, g = p.y / divisor, b = p.z / divisor;
    return (0.2126f * r + 0.7152f * g) + 0.0722f * b;
}

// k_resolve's channel (spt_kernels.hip to_u8): clamp to [0, 1], NaN is 0, truncate to 8 bits
__host__ __device__ inline uint32_t display_u8(float c) {
    c = c < 0.0f ? 0.0f : (1.0f < c ? 1.0f : c);
    if (c != c) c = 0.0f;
    return (uint32_t)(uint8_t)(c * 255.0f);
}

// One colour channel v of a pixel with divisor f through the operator of d.
__host__ __device__ inline uint32_t display_channel(float v, float f, const spt_display& d) {
    float x = v / f;
    x = x * d.exposure;
    if (d.tonemap == SPT_TONEMAP_CLAMP) return display_u8(x);
    x = x > 0.0f ? fminf(x, 65536.0f) : 0.0f;  // NaN and negatives: 0; inf never reaches the operator
    float y;
    if (d.tonemap == SPT_TONEMAP_REINHARD)
        y = x / (1.0f + x);
    else  // SPT_TONEMAP_ACES: the rational fit
        y = (x * (2.51f * x + 0.03f)) / (x * (2.43f * x + 0.59f) + 0.14f);
    return display_u8(y);
}

// One pixel's RGBA8, packed as k_resolve packs it; alpha without exposure or operator.
__host__ __device__ inline uint32_t display_rgba8(float4 a, float f, const spt_display& d) {
    return (display_channel(a.x, f, d) << 24) | (display_channel(a.y, f, d) << 16) | (display_channel(a.z, f, d) << 8) |
           display_u8(a.w / f);
}

// The two forms of k_meter, same counts: kMeterLanes adds one to the wave's LDS
// sub-histogram per lane; kMeterPeel has one lane add the population count of each distinct bin of the wave.
constexpr int kMeterLanes = 0;
constexpr int kMeterPeel = 1;
// the form the library runs (measured, profiles/display_rates.txt)
int meter_default_form();
// counts[0..255] += the histogram of img[0..n) / divisor (the caller zeroes them on the stream first)
void launch_meter(int form, const float4* img, uint64_t n, float divisor, uint32_t* counts, hipStream_t s);
// out[i] = display_rgba8(img[i], divisor, d)
void launch_display(const float4* img, uint64_t n, float divisor, const spt_display& d, uint32_t* out, hipStream_t s);

}  // namespace spt
