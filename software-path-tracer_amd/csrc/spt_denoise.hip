// spt_denoise.hip — the edge-avoiding a-trous filter's kernels for MI355X (gfx950): one launch per level,
// every pixel's 25 taps weighted and summed by spt_atrous.h atrous_pixel (the function spt_atrous_host
// runs on the CPU: the same bits). A translation unit of its own: spt_kernels.hip is the run-time
// compiler's source and stays free of it.
//
// Per level and pixel: 16 B colour + 32 B features per tap read, 16 B written. Two forms, same bits:
//   straight: one thread per pixel, a wave along 64 pixels of a row; every tap a guarded global load
//             (three 16-B loads, contiguous across the wave), served by L2 / the Infinity Cache.
//   tiled:    at step s the pixels of one residue class (x mod s, y mod s) are a sub-image whose taps are
//             its own neighbours: a block takes a 16 x 16 tile of one class plus the two-pixel halo, stages
//             the 20 x 20 records (colour with its compressed luminance, position and material, normal and
//             the pixel's alpha: 48 B, 19.2 KB) in LDS with loads strided by s pixels, and reads every tap
//             from LDS; the luminance's division runs once per staged record, not once per tap.
// atrous_form_of_step picks the form per step from the measurement in profiles/denoise_rates.txt: tiled at
// step 1, straight from step 2 on.
#include "spt_denoise.h"

namespace spt {

namespace {

constexpr int kTile = 16;            // tiled: the block's pixels of one class, kTile x kTile
constexpr int kHalo = 2;             // taps reach two class neighbours each way
constexpr int kTileW = kTile + 2 * kHalo;
constexpr int kTileRecs = kTileW * kTileW;
constexpr int kRowLanes = 64;        // straight: a wave along a row
constexpr int kRowsPerBlock = 4;

template <bool kDiv>
__device__ __forceinline__ float4 mean_colour(float4 c, float divisor) {
    if (kDiv) return make_float4(c.x / divisor, c.y / divisor, c.z / divisor, c.w / divisor);
    return c;
}

template <bool kDiv>
__global__ __launch_bounds__(kRowLanes* kRowsPerBlock) void k_atrous_straight(
    const float4* __restrict__ color, float divisor, const float4* __restrict__ feat_a,
    const float4* __restrict__ feat_b, float4* __restrict__ out, int w, int h, AtrousLevel lv) {
    const int x = (int)(blockIdx.x * kRowLanes + threadIdx.x);
    const int y = (int)(blockIdx.y * kRowsPerBlock + threadIdx.y);
    if (x >= w || y >= h) return;
    const size_t at = (size_t)y * (size_t)w + (size_t)x;
    const float4 c = mean_colour<kDiv>(color[at], divisor);
    const AtrousTap p = atrous_tap(c, feat_a[at], feat_b[at]);
    out[at] = atrous_pixel(p, c.w, x, y, w, h, lv, [&](int, int, int qx, int qy) {
        const size_t q = (size_t)qy * (size_t)w + (size_t)qx;  // (inside the image: atrous_pixel asks for no other)
        return atrous_tap(mean_colour<kDiv>(color[q], divisor), feat_a[q], feat_b[q]);
    });
}

template <bool kDiv>
__global__ __launch_bounds__(kTile* kTile) void k_atrous_tiled(const float4* __restrict__ color, float divisor,
                                                                const float4* __restrict__ feat_a,
                                                                const float4* __restrict__ feat_b,
                                                                float4* __restrict__ out, int w, int h,
                                                                AtrousLevel lv) {
    __shared__ float4 s_c[kTileRecs];  // (r, g, b, lum)
    __shared__ float4 s_a[kTileRecs];  // (P, material)
    __shared__ float4 s_b[kTileRecs];  // (n, the pixel's alpha)
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
        s_c[r] = make_float4(c.x, c.y, c.z, atrous_lum(c.x, c.y, c.z));
        s_a[r] = feat_a[q];
        s_b[r] = make_float4(fb.x, fb.y, fb.z, c.w);
    }
    __syncthreads();
    const int lx = tid % kTile, ly = tid / kTile;
    const int u = u0 + lx, v = v0 + ly;
    if (u >= cw || v >= ch) return;
    auto rec = [&](int r) {
        const float4 c = s_c[r], a = s_a[r], b = s_b[r];
        return AtrousTap{c.x, c.y, c.z, c.w, a.x, a.y, a.z, __float_as_uint(a.w), b.x, b.y, b.z};
    };
    const int centre = (ly + kHalo) * kTileW + lx + kHalo;
    const int x = cx + u * s, y = cy + v * s;
    out[(size_t)y * (size_t)w + (size_t)x] =
        atrous_pixel(rec(centre), s_b[centre].w, x, y, w, h, lv,
                     [&](int i, int j, int, int) { return rec((ly + j) * kTileW + lx + i); });
}

}  // namespace

// Measured on one MI355X, Cornell 1920 x 1080 (profiles/denoise_rates.txt), straight / tiled in us per level:
// step 1: 94.6 / 55.7 (the level that also divides by the frame count: per tap in the straight form, per
// staged record in the tiled one); step 2: 62.0 / 73.4; 4: 64.6 / 116.1; 8: 66.9 / 178.1; 16: 62.0 / 77.4
// (the tiled form's loads are strided by the step and every line is fetched again by each class's blocks).
int atrous_form_of_step(int step) { return step == 1 ? kAtrousTiled : kAtrousStraight; }

void launch_atrous(int form, const float4* color, float divisor, const float4* feat_a, const float4* feat_b,
                   float4* out, uint32_t w, uint32_t h, const AtrousLevel& lv, hipStream_t s) {
    const bool div = divisor != 0.0f;
    if (form == kAtrousTiled) {
        const uint32_t step = (uint32_t)lv.step;
        const uint32_t cw = (w + step - 1) / step, ch = (h + step - 1) / step;  // class 0's sub-image
        const dim3 grid((cw + kTile - 1) / kTile, (ch + kTile - 1) / kTile, step * step);
        if (div) k_atrous_tiled<true><<<grid, kTile * kTile, 0, s>>>(color, divisor, feat_a, feat_b, out, (int)w, (int)h, lv);
        else k_atrous_tiled<false><<<grid, kTile * kTile, 0, s>>>(color, divisor, feat_a, feat_b, out, (int)w, (int)h, lv);
        return;
    }
    const dim3 grid((w + kRowLanes - 1) / kRowLanes, (h + kRowsPerBlock - 1) / kRowsPerBlock);
    const dim3 block(kRowLanes, kRowsPerBlock);
    if (div) k_atrous_straight<true><<<grid, block, 0, s>>>(color, divisor, feat_a, feat_b, out, (int)w, (int)h, lv);
    else k_atrous_straight<false><<<grid, block, 0, s>>>(color, divisor, feat_a, feat_b, out, (int)w, (int)h, lv);
}

}  // namespace spt
