// spt_denoise_guided.hip — the variance-guided a-trous filter's kernels for MI355X (gfx950): one launch for the
// variance plane, then one per level, every pixel by spt_atrous_guided.h's functions (the ones
// spt_atrous_guided_host runs on the CPU: the same bits). A translation unit of its own: spt_denoise.hip and
// spt_kernels.hip stay as they are.
//
// k_guided_variance: 16 B of moments read (the m2 word of each record is used) and 4 B written per pixel. With
//   the prefilter a block takes a 64 x 16 tile: it stages fmaxf(m2 * inv, 0) of the tile and its one-pixel halo
//   in LDS (rows of 66 floats filled by consecutive lanes), then every lane taps its 3 x 3 window there; a wave
//   owns tile rows wave, wave + 4, ..., a lane one column, so every global and LDS access of a wave is one
//   contiguous run. Without it: one thread per pixel, no LDS.
// Per level and pixel: 16 B colour + 4 B variance + 32 B features per tap read, 16 B + 4 B written. Two forms,
// same bits, as spt_denoise.hip's:
//   straight: one thread per pixel, a wave along 64 pixels of a row; every tap a guarded global load.
//   tiled:    a block takes a 16 x 16 tile of one residue class (x mod s, y mod s) plus the two-pixel halo and
//             stages the 20 x 20 records (colour with its linear luminance, position and material, normal and
//             alpha, variance: 52 B, 20.8 KB) in four LDS arrays, consecutive lanes at consecutive records; the
//             luminance is computed once per staged record.
// guided_form_of_step picks the form per step from the measurement in profiles/guided_rates.txt: tiled at
// step 1, straight from step 2 on.
#include "spt_denoise_guided.h"

namespace spt {

namespace {

constexpr int kTile = 16;            // tiled: the block's pixels of one class, kTile x kTile
constexpr int kHalo = 2;             // taps reach two class neighbours each way
constexpr int kTileW = kTile + 2 * kHalo;
constexpr int kTileRecs = kTileW * kTileW;
constexpr int kRowLanes = 64;        // straight: a wave along a row
constexpr int kRowsPerBlock = 4;
constexpr int kVarBlock = 256;       // the variance kernel: four waves over a 64 x 16 tile
constexpr int kVarWaves = kVarBlock / 64;
constexpr int kVarTileW = 64, kVarTileH = 16;
constexpr int kVarHaloW = kVarTileW + 2, kVarHaloH = kVarTileH + 2;

template <bool kDiv>
__device__ __forceinline__ float4 mean_colour(float4 c, float divisor) {
    if (kDiv) return make_float4(c.x / divisor, c.y / divisor, c.z / divisor, c.w / divisor);
    return c;
}

template <bool kPrefilter>
__global__ __launch_bounds__(kVarBlock) void k_guided_variance(const float4* __restrict__ moments,
                                                               float* __restrict__ var, int w, int h, float inv) {
    const int tid = (int)threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int x0 = (int)blockIdx.x * kVarTileW, y0 = (int)blockIdx.y * kVarTileH;
    const int x = x0 + lane;
    if (!kPrefilter) {
#pragma unroll
        for (int k = 0; k < kVarTileH / kVarWaves; ++k) {
            const int y = y0 + wave + k * kVarWaves;
            if (x < w && y < h) {
                const size_t at = (size_t)y * (size_t)w + (size_t)x;
                var[at] = guided_variance0(moments[at].y, inv);
            }
        }
        return;
    }
    __shared__ float s_v[kVarHaloH * kVarHaloW];
    for (int k = tid; k < kVarHaloH * kVarHaloW; k += kVarBlock) {
        const int gx = x0 - 1 + k % kVarHaloW, gy = y0 - 1 + k / kVarHaloW;
        if (gx >= 0 && gx < w && gy >= 0 && gy < h)
            s_v[k] = guided_variance0(moments[(size_t)gy * (size_t)w + (size_t)gx].y, inv);
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kVarTileH / kVarWaves; ++k) {
        const int y = y0 + wave + k * kVarWaves;
        if (x < w && y < h) {
            // (only taps inside the image are read: the halo's other words are never written)
            var[(size_t)y * (size_t)w + (size_t)x] = guided_prefilter_pixel(
                x, y, w, h, [&](int qx, int qy) { return s_v[(qy - y0 + 1) * kVarHaloW + (qx - x0 + 1)]; });
        }
    }
}

template <bool kDiv>
__global__ __launch_bounds__(kRowLanes* kRowsPerBlock) void k_guided_straight(
    const float4* __restrict__ color, float divisor, const float* __restrict__ var, const float4* __restrict__ feat_a,
    const float4* __restrict__ feat_b, float4* __restrict__ out, float* __restrict__ out_var, int w, int h,
    GuidedLevel lv) {
    const int x = (int)(blockIdx.x * kRowLanes + threadIdx.x);
    const int y = (int)(blockIdx.y * kRowsPerBlock + threadIdx.y);
    if (x >= w || y >= h) return;
    const size_t at = (size_t)y * (size_t)w + (size_t)x;
    const float4 c = mean_colour<kDiv>(color[at], divisor);
    const GuidedTap p = guided_tap(c, feat_a[at], feat_b[at], var[at]);
    float v;
    out[at] = guided_pixel(
        p, c.w, x, y, w, h, lv,
        [&](int, int, int qx, int qy) {
            const size_t q = (size_t)qy * (size_t)w + (size_t)qx;  // (inside the image: guided_pixel asks for no other)
            return guided_tap(mean_colour<kDiv>(color[q], divisor), feat_a[q], feat_b[q], var[q]);
        },
        &v);
    out_var[at] = v;
}

template <bool kDiv>
__global__ __launch_bounds__(kTile* kTile) void k_guided_tiled(const float4* __restrict__ color, float divisor,
                                                                const float* __restrict__ var,
                                                                const float4* __restrict__ feat_a,
                                                                const float4* __restrict__ feat_b,
                                                                float4* __restrict__ out, float* __restrict__ out_var,
                                                                int w, int h, GuidedLevel lv) {
    __shared__ float4 s_c[kTileRecs];  // (r, g, b, linear luminance)
    __shared__ float4 s_a[kTileRecs];  // (P, material)
    __shared__ float4 s_b[kTileRecs];  // (n, the pixel's alpha)
    __shared__ float s_v[kTileRecs];   // the variance
    const int s = lv.step;
    const int cx = (int)blockIdx.z % s, cy = (int)blockIdx.z / s;  // the class; its sub-image is cw x ch
    if (cx >= w || cy >= h) return;
    const int cw = (w - cx + s - 1) / s, ch = (h - cy + s - 1) / s;
    const int u0 = (int)blockIdx.x * kTile, v0 = (int)blockIdx.y * kTile;
    if (u0 >= cw || v0 >= ch) return;  // (uniform: the grid is sized for class 0, the largest)
    const int tid = (int)threadIdx.x;
    for (int r = tid; r < kTileRecs; r += kTile * kTile) {
        const int u = u0 - kHalo + r % kTileW, v = v0 - kHalo + r / kTileW;
        if (u < 0 || v < 0 || u >= cw || v >= ch) continue;  // outside the image: no tap reads it
        const size_t q = (size_t)(cy + v * s) * (size_t)w + (size_t)(cx + u * s);
        const float4 c = mean_colour<kDiv>(color[q], divisor);
        const float4 fb = feat_b[q];
        s_c[r] = make_float4(c.x, c.y, c.z, guided_lum(c.x, c.y, c.z));
        s_a[r] = feat_a[q];
        s_b[r] = make_float4(fb.x, fb.y, fb.z, c.w);
        s_v[r] = var[q];
    }
    __syncthreads();
    const int lx = tid % kTile, ly = tid / kTile;
    const int u = u0 + lx, v = v0 + ly;
    if (u >= cw || v >= ch) return;
    auto rec = [&](int r) {
        const float4 c = s_c[r], a = s_a[r], b = s_b[r];
        return GuidedTap{c.x, c.y, c.z, c.w, a.x, a.y, a.z, __float_as_uint(a.w), b.x, b.y, b.z, s_v[r]};
    };
    const int centre = (ly + kHalo) * kTileW + lx + kHalo;
    const int x = cx + u * s, y = cy + v * s;
    const size_t at = (size_t)y * (size_t)w + (size_t)x;
    float pv;
    out[at] = guided_pixel(
        rec(centre), s_b[centre].w, x, y, w, h, lv,
        [&](int i, int j, int, int) { return rec((ly + j) * kTileW + lx + i); }, &pv);
    out_var[at] = pv;
}

}  // namespace

// Measured on one MI355X, Cornell 1920 x 1080 (profiles/guided_rates.txt), straight / tiled in us per level:
// step 1 with k_guided_variance: 103.0 / 72.1; step 2: 67.0 / 84.5; 4: 67.6 / 134.2; 8: 72.6 / 208.3; 16: 66.1 / 85.5:
// spt_denoise.hip's choice again, for its reasons.
int guided_form_of_step(int step) { return step == 1 ? kGuidedTiled : kGuidedStraight; }

void launch_guided_variance(const float4* moments, float* var, uint32_t w, uint32_t h, float inv, bool prefilter,
                            hipStream_t s) {
    if (w == 0 || h == 0) return;
    const dim3 grid((w + kVarTileW - 1) / kVarTileW, (h + kVarTileH - 1) / kVarTileH);
    if (prefilter) k_guided_variance<true><<<grid, kVarBlock, 0, s>>>(moments, var, (int)w, (int)h, inv);
    else k_guided_variance<false><<<grid, kVarBlock, 0, s>>>(moments, var, (int)w, (int)h, inv);
}

void launch_guided_level(int form, const float4* color, float divisor, const float* var, const float4* feat_a,
                         const float4* feat_b, float4* out, float* out_var, uint32_t w, uint32_t h,
                         const GuidedLevel& lv, hipStream_t s) {
    const bool div = divisor != 0.0f;
    if (form == kGuidedTiled) {
        const uint32_t step = (uint32_t)lv.step;
        const uint32_t cw = (w + step - 1) / step, ch = (h + step - 1) / step;  // class 0's sub-image
        const dim3 grid((cw + kTile - 1) / kTile, (ch + kTile - 1) / kTile, step * step);
        if (div) k_guided_tiled<true><<<grid, kTile * kTile, 0, s>>>(color, divisor, var, feat_a, feat_b, out, out_var, (int)w, (int)h, lv);
        else k_guided_tiled<false><<<grid, kTile * kTile, 0, s>>>(color, divisor, var, feat_a, feat_b, out, out_var, (int)w, (int)h, lv);
        return;
    }
    const dim3 grid((w + kRowLanes - 1) / kRowLanes, (h + kRowsPerBlock - 1) / kRowsPerBlock);
    const dim3 block(kRowLanes, kRowsPerBlock);
    if (div) k_guided_straight<true><<<grid, block, 0, s>>>(color, divisor, var, feat_a, feat_b, out, out_var, (int)w, (int)h, lv);
    else k_guided_straight<false><<<grid, block, 0, s>>>(color, divisor, var, feat_a, feat_b, out, out_var, (int)w, (int)h, lv);
}

}  // namespace spt
