// spt_display.hip — the luminance meter's and the display transform's kernels for MI355X (gfx950), every pixel
// by spt_display.h's functions (the ones spt_luminance_histogram_host and spt_display_host run on the CPU: the
// same bits). A translation unit of its own: spt_kernels.hip is the run-time compiler's source and stays free
// of it.
//
// k_meter: 16 B read per pixel, 1 KB written. A capped grid strides over the image, a thread loading four pixels
// before it bins them; a block sums into LDS sub-histograms private to each of its four waves (4 KB), then adds
// its non-zero bins to the 256 global words with device-scope integer atomics: exact whatever the order. Two
// forms of the LDS sum, same counts:
//   lanes: every lane adds one to its bin (ds_add_u32), whether or not lanes of the wave share a bin.
//   peel:  the wave takes its first pending lane's bin, ballots the lanes that hold the same one and has one
//          lane add their number; it repeats until no lane is pending. A flat region costs one or two adds per
//          wave, a noisy one up to 64 rounds.
// k_display: k_resolve with display_rgba8: 16 B read and 4 B written per pixel.
#include "spt_display.h"

namespace spt {

namespace {

constexpr int kMeterBlock = 256;  // four waves
constexpr int kMeterWaves = kMeterBlock / 64;
constexpr int kMeterUnroll = 4;             // pixels a thread loads before it bins them
// One block per CU, the rest of the image by the stride: every block ends with an atomic per occupied bin on the
// same 256 words. In a one-off sweep of this cap the kernel's time grew by about 10 ns per block
// from 256 blocks up, whatever the image, and rose again below 192: the grid is as small as still streams.
constexpr uint32_t kMeterMaxBlocks = 256;
constexpr int kDisplayBlock = 256;
constexpr uint64_t kDisplayMaxBlocks = 0x7fffffffull;

static_assert(SPT_METER_BINS == kMeterBlock, "a block's thread per bin zeroes and flushes the histogram");

// One pixel's bin into the wave's sub-histogram h, for the lanes that call it together.
template <int kForm>
__device__ __forceinline__ void meter_add(uint32_t* h, uint32_t lane, uint32_t bin) {
    if (kForm == kMeterLanes) {
        atomicAdd(&h[bin], 1u);
        return;
    }
    // (lanes that hold no pixel are not here: the ballots count the active lanes only)
    bool pending = true;
    while (pending) {
        const uint32_t b = (uint32_t)__builtin_amdgcn_readfirstlane((int)bin);  // the first pending lane's
        const uint64_t same = __ballot(bin == b);
        if (bin == b) {
            if (lane == (uint32_t)(__ffsll((unsigned long long)same) - 1)) atomicAdd(&h[b], (uint32_t)__popcll(same));
            pending = false;
        }
    }
}

template <int kForm>
__global__ __launch_bounds__(kMeterBlock) void k_meter(const float4* __restrict__ img, uint64_t n, float divisor,
                                                       uint32_t* __restrict__ counts) {
    __shared__ uint32_t s_h[kMeterWaves][SPT_METER_BINS];
    const uint32_t tid = threadIdx.x;
    for (int w = 0; w < kMeterWaves; ++w) s_h[w][tid] = 0u;
    __syncthreads();
    uint32_t* h = s_h[tid >> 6];
    const uint32_t lane = tid & 63u;
    // a block takes kMeterUnroll runs of 256 consecutive pixels per step, their loads issued together
    const uint64_t step = (uint64_t)kMeterBlock * kMeterUnroll;
    for (uint64_t base = (uint64_t)blockIdx.x * step + tid; base < n; base += (uint64_t)gridDim.x * step) {
        float4 p[kMeterUnroll];
#pragma unroll
        for (int k = 0; k < kMeterUnroll; ++k) {
            const uint64_t i = base + (uint64_t)k * kMeterBlock;
            if (i < n) p[k] = img[i];
        }
#pragma unroll
        for (int k = 0; k < kMeterUnroll; ++k)
            if (base + (uint64_t)k * kMeterBlock < n) meter_add<kForm>(h, lane, meter_bin(pixel_luminance(p[k], divisor)));
    }
    __syncthreads();
    uint32_t total = 0u;
    for (int w = 0; w < kMeterWaves; ++w) total += s_h[w][tid];
    if (total) atomicAdd(&counts[tid], total);
}

__global__ __launch_bounds__(kDisplayBlock) void k_display(const float4* __restrict__ img, uint64_t n, float divisor,
                                                           spt_display d, uint32_t* __restrict__ out) {
    const uint64_t stride = (uint64_t)gridDim.x * kDisplayBlock;  // (one pass for any image of < 2^39 pixels)
    for (uint64_t i = (uint64_t)blockIdx.x * kDisplayBlock + threadIdx.x; i < n; i += stride)
        out[i] = display_rgba8(img[i], divisor, d);
}

}  // namespace

// Measured on one MI355X at 1920 x 1080 (profiles/display_rates.txt): the LDS add per lane
// costs the same on a converged Cornell image, whose two fullest bins hold a third of the pixels, as on a
// uniformly random one (10-12 us), and the peel is never faster: 16-19 us on Cornell, 72 us on the random image.
int meter_default_form() { return kMeterLanes; }

void launch_meter(int form, const float4* img, uint64_t n, float divisor, uint32_t* counts, hipStream_t s) {
    if (n == 0) return;
    const uint64_t per_block = (uint64_t)kMeterBlock * kMeterUnroll;
    const uint64_t blocks = (n + per_block - 1) / per_block;
    const uint32_t grid = (uint32_t)(blocks < kMeterMaxBlocks ? blocks : kMeterMaxBlocks);
    if (form == kMeterPeel) k_meter<kMeterPeel><<<grid, kMeterBlock, 0, s>>>(img, n, divisor, counts);
    else k_meter<kMeterLanes><<<grid, kMeterBlock, 0, s>>>(img, n, divisor, counts);
}

void launch_display(const float4* img, uint64_t n, float divisor, const spt_display& d, uint32_t* out, hipStream_t s) {
    if (n == 0) return;
    const uint64_t blocks = (n + kDisplayBlock - 1) / kDisplayBlock;
    const uint32_t grid = (uint32_t)(blocks < kDisplayMaxBlocks ? blocks : kDisplayMaxBlocks);
    k_display<<<grid, kDisplayBlock, 0, s>>>(img, n, divisor, d, out);
}

}  // namespace spt
