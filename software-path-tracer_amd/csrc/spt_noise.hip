// spt_noise.hip — the noise estimate's kernels for MI355X (gfx950), every pixel by spt_noise.h's functions (the
// ones spt_host.cpp's spt_noise_update_host and spt_noise_meter_host run on the CPU: the same bits). A translation unit of its
// own: spt_kernels.hip is the run-time compiler's source and stays free of it.
//
// k_noise_update: a streaming pass, 16 B of accumulation and 16 B of state read and 16 B written per pixel. A
// capped grid strides over the image; a thread issues the eight 16-byte loads of four pixels 256 apart before it
// folds them.
// k_noise_meter (radius 0): 16 B of state read and 4 B of e2 written per pixel, binned as k_meter bins (spt_display.hip):
// an LDS sub-histogram per wave, one add per lane, one device-scope integer atomic per occupied bin per block,
// the grid capped at 256 blocks for the sake of those atomics' serialisation per word.
// k_noise_meter_pooled<1|2>: the same over a pooled window, in tiles of 64 x 16 pixels: a wave owns tile rows
// wave, wave + 4, ..., a lane one column. The block first stages the tile's (mean, m2) pairs with their halo in
// LDS (8 B per record, rows of 64 + 2 * radius records filled by consecutive lanes), then taps LDS, so every
// global and LDS access of a wave is one contiguous run.
#include "spt_noise.h"

namespace spt {

namespace {

constexpr int kNoiseBlock = 256;  // four waves
constexpr int kNoiseWaves = kNoiseBlock / 64;
constexpr int kNoiseUnroll = 4;  // pixels a thread loads before it folds or bins them
// k_noise_update has no shared words to flush: eight blocks per CU hide the latency of its 48 B per pixel
constexpr uint32_t kUpdateMaxBlocks = 2048;
constexpr uint32_t kMeterMaxBlocks = 256;  // (k_meter's cap: every block ends on the same 256 words)
// The pooled kernel waits for its tile between two barriers, so one block per CU leaves the CU idle meanwhile:
// four per CU. In a one-off sweep (profiles/noise_meter_grid_sweep.txt) radius 1 took 43 us at 256 blocks, 27 at
// 512, 24 at 768 and 1024, 25 at 2048, where the flush into the 256 global words shows again.
constexpr uint32_t kPooledMaxBlocks = 1024;
constexpr int kTileW = 64, kTileH = 16;    // the pooled kernel's tile: a lane per column, four rows per wave

static_assert(SPT_NOISE_BINS == kNoiseBlock, "a block's thread per bin zeroes and flushes the histogram");

__global__ __launch_bounds__(kNoiseBlock) void k_noise_update(const float4* __restrict__ accum,
                                                              float4* __restrict__ state, uint64_t n, NoiseBatch b) {
    const uint64_t step = (uint64_t)kNoiseBlock * kNoiseUnroll;
    for (uint64_t base = (uint64_t)blockIdx.x * step + threadIdx.x; base < n; base += (uint64_t)gridDim.x * step) {
        float4 a[kNoiseUnroll], s[kNoiseUnroll];
#pragma unroll
        for (int k = 0; k < kNoiseUnroll; ++k) {
            const uint64_t i = base + (uint64_t)k * kNoiseBlock;
            if (i < n) {
                a[k] = accum[i];
                s[k] = state[i];
            }
        }
#pragma unroll
        for (int k = 0; k < kNoiseUnroll; ++k) {
            const uint64_t i = base + (uint64_t)k * kNoiseBlock;
            if (i < n) state[i] = noise_update_pixel(a[k], s[k], b);
        }
    }
}

// the block's sub-histograms into the 256 global words (every thread of the block calls it)
__device__ __forceinline__ void flush_bins(uint32_t (*s_h)[SPT_NOISE_BINS], uint32_t* __restrict__ counts) {
    __syncthreads();
    uint32_t total = 0u;
    for (int w = 0; w < kNoiseWaves; ++w) total += s_h[w][threadIdx.x];
    if (total) atomicAdd(&counts[threadIdx.x], total);
}

__global__ __launch_bounds__(kNoiseBlock) void k_noise_meter(const float4* __restrict__ state, uint64_t n, float inv,
                                                             float dark_floor, uint32_t* __restrict__ counts,
                                                             float* __restrict__ e2) {
    __shared__ uint32_t s_h[kNoiseWaves][SPT_NOISE_BINS];
    const uint32_t tid = threadIdx.x;
    for (int w = 0; w < kNoiseWaves; ++w) s_h[w][tid] = 0u;
    __syncthreads();
    uint32_t* h = s_h[tid >> 6];
    const uint64_t step = (uint64_t)kNoiseBlock * kNoiseUnroll;
    for (uint64_t base = (uint64_t)blockIdx.x * step + tid; base < n; base += (uint64_t)gridDim.x * step) {
        float4 s[kNoiseUnroll];
#pragma unroll
        for (int k = 0; k < kNoiseUnroll; ++k) {
            const uint64_t i = base + (uint64_t)k * kNoiseBlock;
            if (i < n) s[k] = state[i];
        }
#pragma unroll
        for (int k = 0; k < kNoiseUnroll; ++k) {
            const uint64_t i = base + (uint64_t)k * kNoiseBlock;
            if (i < n) {
                const float e = noise_e2(s[k].x, s[k].y, inv, dark_floor);
                if (e2) e2[i] = e;
                atomicAdd(&h[noise_bin(e)], 1u);
            }
        }
    }
    flush_bins(s_h, counts);
}

template <int kRadius>
__global__ __launch_bounds__(kNoiseBlock) void k_noise_meter_pooled(const float4* __restrict__ state, int width,
                                                                    int height, float inv, float dark_floor,
                                                                    uint32_t* __restrict__ counts,
                                                                    float* __restrict__ e2) {
    constexpr int kHaloW = kTileW + 2 * kRadius, kHaloH = kTileH + 2 * kRadius;
    __shared__ uint32_t s_h[kNoiseWaves][SPT_NOISE_BINS];
    __shared__ float2 s_tile[kHaloH * kHaloW];
    const int tid = (int)threadIdx.x;
    for (int w = 0; w < kNoiseWaves; ++w) s_h[w][tid] = 0u;
    __syncthreads();
    uint32_t* h = s_h[tid >> 6];
    const int lane = tid & 63, wave = tid >> 6;
    // (mean, m2) are the first 8 bytes of a pixel's 16-byte record
    const float2* __restrict__ pairs = (const float2*)state;
    const int tiles_x = (width + kTileW - 1) / kTileW, tiles_y = (height + kTileH - 1) / kTileH;
    for (int tile = (int)blockIdx.x; tile < tiles_x * tiles_y; tile += (int)gridDim.x) {
        const int x0 = (tile % tiles_x) * kTileW, y0 = (tile / tiles_x) * kTileH;
        __syncthreads();  // (the last tile's taps are done)
        for (int k = tid; k < kHaloH * kHaloW; k += kNoiseBlock) {
            const int gx = x0 - kRadius + k % kHaloW, gy = y0 - kRadius + k / kHaloW;
            if (gx >= 0 && gx < width && gy >= 0 && gy < height) s_tile[k] = pairs[2 * ((size_t)gy * width + gx)];
        }
        __syncthreads();
        const int x = x0 + lane;
#pragma unroll
        for (int k = 0; k < kTileH / kNoiseWaves; ++k) {
            const int y = y0 + wave + k * kNoiseWaves;
            if (x < width && y < height) {
                // (only taps inside the image are read: the halo's other records are never written)
                const float e = noise_pooled_e2(x, y, width, height, kRadius, inv, dark_floor, [&](int tx, int ty) {
                    return s_tile[(ty - y0 + kRadius) * kHaloW + (tx - x0 + kRadius)];
                });
                if (e2) e2[(size_t)y * width + x] = e;
                atomicAdd(&h[noise_bin(e)], 1u);
            }
        }
    }
    flush_bins(s_h, counts);
}

template <int kRadius>
void launch_pooled(const float4* state, uint32_t width, uint32_t height, float inv, float dark_floor,
                   uint32_t* counts, float* e2, hipStream_t s) {
    const uint64_t tiles = (uint64_t)((width + kTileW - 1) / kTileW) * ((height + kTileH - 1) / kTileH);
    const uint32_t grid = (uint32_t)(tiles < kPooledMaxBlocks ? tiles : kPooledMaxBlocks);
    k_noise_meter_pooled<kRadius><<<grid, kNoiseBlock, 0, s>>>(state, (int)width, (int)height, inv, dark_floor, counts, e2);
}

}  // namespace

void launch_noise_update(const float4* accum, float4* state, uint64_t n, NoiseBatch b, hipStream_t s) {
    if (n == 0) return;
    const uint64_t per_block = (uint64_t)kNoiseBlock * kNoiseUnroll;
    const uint64_t blocks = (n + per_block - 1) / per_block;
    const uint32_t grid = (uint32_t)(blocks < kUpdateMaxBlocks ? blocks : kUpdateMaxBlocks);
    k_noise_update<<<grid, kNoiseBlock, 0, s>>>(accum, state, n, b);
}

void launch_noise_meter(const float4* state, uint32_t width, uint32_t height, int radius, float inv,
                        float dark_floor, uint32_t* counts, float* e2, hipStream_t s) {
    const uint64_t n = (uint64_t)width * height;
    if (n == 0) return;
    if (radius == 0) {
        const uint64_t per_block = (uint64_t)kNoiseBlock * kNoiseUnroll;
        const uint64_t blocks = (n + per_block - 1) / per_block;
        const uint32_t grid = (uint32_t)(blocks < kMeterMaxBlocks ? blocks : kMeterMaxBlocks);
        k_noise_meter<<<grid, kNoiseBlock, 0, s>>>(state, n, inv, dark_floor, counts, e2);
    } else if (radius == 1) {
        launch_pooled<1>(state, width, height, inv, dark_floor, counts, e2, s);
    } else {
        launch_pooled<2>(state, width, height, inv, dark_floor, counts, e2, s);
    }
}

}  // namespace spt
