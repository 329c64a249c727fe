// spt_reproject.hip — temporal reprojection's kernels for MI355X (gfx950): the capture and the blend of a
// view's image with its history (streaming), and the gather that maps a captured view into the current one,
// every pixel by spt_reproject.h's functions (the ones spt_reproject_host runs on the CPU: the same bits).
// A translation unit of its own, as spt_denoise.hip: spt_kernels.hip is the run-time compiler's source.
//
// Compulsory traffic per pixel: the gather reads 32 B of current features and writes 16 B, and the captured
// view it reads is 48 B per pixel (each of a pixel's four taps is a neighbour's too: L2 serves the repeats);
// the blend reads 32 B and writes 16 B. All loads and stores are 16 B.
#include "spt_reproject.h"

namespace spt {

namespace {

constexpr int kRowLanes = 64;  // a wave along 64 pixels of a row, as the straight a-trous form
constexpr int kRowsPerBlock = 4;
constexpr int kStreamBlock = 256;

// kLayout < 0: no capture, out is the blended image. Otherwise `out` is the captured view in that layout.
template <int kLayout, bool kHist>
__global__ __launch_bounds__(kStreamBlock) void k_history_blend(const float4* __restrict__ accum, float frames,
                                                                const float4* __restrict__ hist,
                                                                const float4* __restrict__ feat_a,
                                                                const float4* __restrict__ feat_b,
                                                                float4* __restrict__ out, uint32_t pixels) {
    const uint32_t at = blockIdx.x * kStreamBlock + threadIdx.x;
    if (at >= pixels) return;
    const float4 h = kHist ? hist[at] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const float4 c = history_blend_pixel<(kLayout >= 0)>(accum[at], frames, h);
    if (kLayout < 0) {
        out[at] = c;
    } else if (kLayout == kHistoryPlanes) {
        out[at] = c;
        out[(size_t)pixels + at] = feat_a[at];
        out[2 * (size_t)pixels + at] = feat_b[at];
    } else {
        out[3 * (size_t)at] = feat_a[at];
        out[3 * (size_t)at + 1] = feat_b[at];
        out[3 * (size_t)at + 2] = c;
    }
}

template <int kLayout>
__global__ __launch_bounds__(kRowLanes* kRowsPerBlock) void k_reproject(
    const float4* __restrict__ feat_a, const float4* __restrict__ feat_b, const float4* __restrict__ view,
    float4* __restrict__ out, int w, int h, ReprojectView v, spt_reproject_params p,
    const uint32_t* __restrict__ reusable, uint32_t n_materials) {
    const int x = (int)(blockIdx.x * kRowLanes + threadIdx.x);
    const int y = (int)(blockIdx.y * kRowsPerBlock + threadIdx.y);
    if (x >= w || y >= h) return;
    const size_t at = (size_t)y * (size_t)w + (size_t)x;
    const size_t n = (size_t)w * (size_t)h;
    // (q is inside the image: reproject_pixel asks for no other)
    if (kLayout == kHistoryPlanes)
        out[at] = reproject_pixel(
            feat_a[at], feat_b[at], w, h, v, p, reusable, n_materials, [&](size_t q) { return view[n + q]; },
            [&](size_t q) { return view[2 * n + q]; }, [&](size_t q) { return view[q]; });
    else
        out[at] = reproject_pixel(
            feat_a[at], feat_b[at], w, h, v, p, reusable, n_materials, [&](size_t q) { return view[3 * q]; },
            [&](size_t q) { return view[3 * q + 1]; }, [&](size_t q) { return view[3 * q + 2]; });
}

}  // namespace

void launch_history_capture(int layout, const float4* accum, float frames, const float4* hist, const float4* feat_a,
                            const float4* feat_b, float4* view, uint32_t pixels, hipStream_t s) {
    const uint32_t grid = (pixels + kStreamBlock - 1) / kStreamBlock;
    if (layout == kHistoryRecords) {
        if (hist) k_history_blend<kHistoryRecords, true><<<grid, kStreamBlock, 0, s>>>(accum, frames, hist, feat_a, feat_b, view, pixels);
        else k_history_blend<kHistoryRecords, false><<<grid, kStreamBlock, 0, s>>>(accum, frames, hist, feat_a, feat_b, view, pixels);
    } else {
        if (hist) k_history_blend<kHistoryPlanes, true><<<grid, kStreamBlock, 0, s>>>(accum, frames, hist, feat_a, feat_b, view, pixels);
        else k_history_blend<kHistoryPlanes, false><<<grid, kStreamBlock, 0, s>>>(accum, frames, hist, feat_a, feat_b, view, pixels);
    }
}

void launch_history_blend(const float4* accum, float frames, const float4* hist, float4* out, uint32_t pixels,
                          hipStream_t s) {
    const uint32_t grid = (pixels + kStreamBlock - 1) / kStreamBlock;
    if (hist) k_history_blend<-1, true><<<grid, kStreamBlock, 0, s>>>(accum, frames, hist, nullptr, nullptr, out, pixels);
    else k_history_blend<-1, false><<<grid, kStreamBlock, 0, s>>>(accum, frames, hist, nullptr, nullptr, out, pixels);
}

void launch_reproject(int layout, const float4* feat_a, const float4* feat_b, const float4* view, float4* out, uint32_t w,
                      uint32_t h, const ReprojectView& v, const spt_reproject_params& p, const uint32_t* reusable,
                      uint32_t n_materials, hipStream_t s) {
    const dim3 grid((w + kRowLanes - 1) / kRowLanes, (h + kRowsPerBlock - 1) / kRowsPerBlock);
    const dim3 block(kRowLanes, kRowsPerBlock);
    if (layout == kHistoryRecords)
        k_reproject<kHistoryRecords><<<grid, block, 0, s>>>(feat_a, feat_b, view, out, (int)w, (int)h, v, p, reusable, n_materials);
    else
        k_reproject<kHistoryPlanes><<<grid, block, 0, s>>>(feat_a, feat_b, view, out, (int)w, (int)h, v, p, reusable, n_materials);
}

}  // namespace spt
