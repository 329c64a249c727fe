// Issue cost of single VALU instructions on gfx950, as multiples of v_fma_f32's (run by
// scripts/valu_issue_cost.py, which compiles this file with hipcc --offload-arch=gfx950).
//
// Per instruction one kernel: every lane keeps kAcc independent accumulators and a trip of the loop issues
// kAcc * kRep instructions on them in turn (inline asm, so nothing is combined, hoisted or strength-reduced;
// consecutive instructions never depend on one another, each accumulator's chain is kAcc instructions long). The
// accumulators are summed and stored at the end, so no chain is dead. Each kernel runs at one and at seven waves per
// SIMD on every CU: blocks of 256 threads (a wave per SIMD), as many blocks as the device holds at once at the
// wanted occupancy, which dynamic LDS enforces (a block asks for 1 / 1 or 1 / 7 of a CU's LDS, so no CU takes more).
// The time is the smallest of kRuns event pairs; the figure is the time per instruction of one wave, in ns, and
// its ratio to v_fma_f32's at the same occupancy.
//
//   valu_issue_cost [trips]      prints one line per (instruction, waves per SIMD)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CHECK(x)                                                                                   \
    do {                                                                                           \
        hipError_t e_ = (x);                                                                       \
        if (e_ != hipSuccess) {                                                                    \
            std::fprintf(stderr, "%s:%d: %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_)); \
            std::exit(1);                                                                          \
        }                                                                                          \
    } while (0)

constexpr int kAcc = 8;   // independent accumulators per lane
constexpr int kRep = 8;   // rounds over them per trip: 64 instructions per trip
constexpr int kRuns = 5;  // timed launches per figure (the smallest counts)

// (the last four are not in question: plain two- and three-operand instructions beside the unit, as a cross-check)
enum Op { kFmaF32, kMulLoU32, kMulHiU32, kMadU64U32, kMadU32U24, kMulU32U24, kLshlAddU64, kFmaF64, kMinF64, kRcpF32,
          kSqrtF32, kAddF32, kMulF32, kAddU32, kLshlAddU32, kOps };
static const char* const kNames[kOps] = {"v_fma_f32", "v_mul_lo_u32", "v_mul_hi_u32", "v_mad_u64_u32", "v_mad_u32_u24",
                                         "v_mul_u32_u24", "v_lshl_add_u64", "v_fma_f64", "v_min_f64", "v_rcp_f32",
                                         "v_sqrt_f32", "v_add_f32", "v_mul_f32", "v_add_u32", "v_lshl_add_u32"};

template <int kOp>
__global__ __launch_bounds__(256) void k_chain(uint32_t* __restrict__ out, uint32_t trips, uint32_t seed) {
    extern __shared__ uint32_t s_pad[];  // occupancy only
    const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t sum = 0;
    if constexpr (kOp == kFmaF32 || kOp == kRcpF32 || kOp == kSqrtF32 || kOp == kAddF32 || kOp == kMulF32) {
        float a[kAcc];
        const float m = 0.999f + 1e-6f * (float)(seed & 7u), c = 0.001f;
        for (int i = 0; i < kAcc; ++i) a[i] = 1.0f + 0.125f * (float)((tid + i + seed) & 7u);
        for (uint32_t t = 0; t < trips; ++t) {
#pragma unroll
            for (int r = 0; r < kRep; ++r)
#pragma unroll
                for (int i = 0; i < kAcc; ++i) {
                    if constexpr (kOp == kFmaF32) asm volatile("v_fma_f32 %0, %0, %1, %2" : "+v"(a[i]) : "v"(m), "v"(c));
                    if constexpr (kOp == kRcpF32) asm volatile("v_rcp_f32 %0, %0" : "+v"(a[i]));
                    if constexpr (kOp == kSqrtF32) asm volatile("v_sqrt_f32 %0, %0" : "+v"(a[i]));
                    if constexpr (kOp == kAddF32) asm volatile("v_add_f32 %0, %0, %1" : "+v"(a[i]) : "v"(c));
                    if constexpr (kOp == kMulF32) asm volatile("v_mul_f32 %0, %0, %1" : "+v"(a[i]) : "v"(m));
                }
        }
        for (int i = 0; i < kAcc; ++i) sum += __float_as_uint(a[i]);
    } else if constexpr (kOp == kFmaF64 || kOp == kMinF64) {
        double a[kAcc];
        const double m = 0.999 + 1e-6 * (double)(seed & 7u), c = 0.001;
        for (int i = 0; i < kAcc; ++i) a[i] = 1.0 + 0.125 * (double)((tid + i + seed) & 7u);
        for (uint32_t t = 0; t < trips; ++t) {
#pragma unroll
            for (int r = 0; r < kRep; ++r)
#pragma unroll
                for (int i = 0; i < kAcc; ++i) {
                    if constexpr (kOp == kFmaF64) asm volatile("v_fma_f64 %0, %0, %1, %2" : "+v"(a[i]) : "v"(m), "v"(c));
                    if constexpr (kOp == kMinF64) asm volatile("v_min_f64 %0, %0, %1" : "+v"(a[i]) : "v"(m));
                }
        }
        for (int i = 0; i < kAcc; ++i) sum += (uint32_t)__double2loint(a[i]) + (uint32_t)__double2hiint(a[i]);
    } else if constexpr (kOp == kMadU64U32 || kOp == kLshlAddU64) {
        unsigned long long a[kAcc];
        const uint32_t m = 747796405u + seed, c = 2891336453u ^ tid;
        const unsigned long long c64 = ((unsigned long long)m << 32) | c;
        for (int i = 0; i < kAcc; ++i) a[i] = (unsigned long long)(tid + i) * 0x9E3779B97F4A7C15ull + seed;
        for (uint32_t t = 0; t < trips; ++t) {
#pragma unroll
            for (int r = 0; r < kRep; ++r)
#pragma unroll
                for (int i = 0; i < kAcc; ++i) {
                    if constexpr (kOp == kMadU64U32)
                        asm volatile("v_mad_u64_u32 %0, vcc, %1, %2, %0" : "+v"(a[i]) : "v"(m), "v"(c) : "vcc");
                    if constexpr (kOp == kLshlAddU64) asm volatile("v_lshl_add_u64 %0, %0, 1, %1" : "+v"(a[i]) : "v"(c64));
                }
        }
        for (int i = 0; i < kAcc; ++i) sum += (uint32_t)a[i] + (uint32_t)(a[i] >> 32);
    } else {
        uint32_t a[kAcc];
        const uint32_t m = 747796405u + 2u * seed, c = 2891336453u ^ tid;
        for (int i = 0; i < kAcc; ++i) a[i] = (tid + i) * 277803737u + seed;
        for (uint32_t t = 0; t < trips; ++t) {
#pragma unroll
            for (int r = 0; r < kRep; ++r)
#pragma unroll
                for (int i = 0; i < kAcc; ++i) {
                    if constexpr (kOp == kMulLoU32) asm volatile("v_mul_lo_u32 %0, %0, %1" : "+v"(a[i]) : "v"(m));
                    if constexpr (kOp == kMulHiU32) asm volatile("v_mul_hi_u32 %0, %0, %1" : "+v"(a[i]) : "v"(m));
                    if constexpr (kOp == kMadU32U24) asm volatile("v_mad_u32_u24 %0, %0, %1, %2" : "+v"(a[i]) : "v"(m), "v"(c));
                    if constexpr (kOp == kMulU32U24) asm volatile("v_mul_u32_u24 %0, %0, %1" : "+v"(a[i]) : "v"(m));
                    if constexpr (kOp == kAddU32) asm volatile("v_add_u32 %0, %0, %1" : "+v"(a[i]) : "v"(m));
                    if constexpr (kOp == kLshlAddU32) asm volatile("v_lshl_add_u32 %0, %0, 1, %1" : "+v"(a[i]) : "v"(c));
                }
        }
        for (int i = 0; i < kAcc; ++i) sum += a[i];
    }
    out[tid] = sum;
}

template <int kOp>
static float time_ms(uint32_t* out, uint32_t blocks, uint32_t lds, uint32_t trips) {
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_chain<kOp>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    float best = 1e30f;
    for (int run = 0; run <= kRuns; ++run) {  // (run 0: the code object's load, not timed)
        CHECK(hipEventRecord(e0, nullptr));
        hipLaunchKernelGGL(k_chain<kOp>, dim3(blocks), dim3(256), lds, nullptr, out, run ? trips : 16u, (uint32_t)run);
        CHECK(hipGetLastError());
        CHECK(hipEventRecord(e1, nullptr));
        CHECK(hipEventSynchronize(e1));
        float ms = 0.f;
        CHECK(hipEventElapsedTime(&ms, e0, e1));
        if (run) best = std::min(best, ms);
    }
    CHECK(hipEventDestroy(e0));
    CHECK(hipEventDestroy(e1));
    return best;
}

template <int kOp = 0>
static void all_ops(uint32_t* out, uint32_t blocks, uint32_t lds, uint32_t trips, float* ms) {
    if constexpr (kOp < kOps) {
        ms[kOp] = time_ms<kOp>(out, blocks, lds, trips);
        all_ops<kOp + 1>(out, blocks, lds, trips, ms);
    }
}

int main(int argc, char** argv) {
    const uint32_t trips = argc > 1 ? (uint32_t)std::strtoul(argv[1], nullptr, 10) : 8192u;
    hipDeviceProp_t prop;
    CHECK(hipGetDeviceProperties(&prop, 0));
    const uint32_t cus = (uint32_t)prop.multiProcessorCount;
    const uint32_t lds_cu = (uint32_t)prop.maxSharedMemoryPerMultiProcessor;
    std::printf("# %s: %u CUs, %u B LDS per CU, %d MHz; %u trips of %d instructions per wave, the smallest of %d launches\n",
                prop.name, cus, lds_cu, prop.clockRate / 1000, trips, kAcc * kRep, kRuns);
    uint32_t* out = nullptr;
    CHECK(hipMalloc(&out, (size_t)cus * 7u * 256u * sizeof(uint32_t)));
    // the clocks settle under load before anything is timed (the first figure otherwise carries their ramp)
    for (int i = 0; i < 40; ++i) hipLaunchKernelGGL(k_chain<kFmaF32>, dim3(cus * 4u), dim3(256), 0, nullptr, out, trips, 0u);
    CHECK(hipDeviceSynchronize());
    std::printf("# instruction waves_per_simd ms ns_per_instruction_per_wave x_v_fma_f32\n");
    for (uint32_t wps : {1u, 7u}) {
        // a block's LDS: more than 1 / (wps + 1) of the CU's, so wps blocks fit and wps + 1 do not
        const uint32_t lds = std::min(lds_cu / wps, (uint32_t)prop.sharedMemPerBlock) & ~255u;
        if ((wps + 1u) * lds <= lds_cu)  // (a block may not ask for enough: the spread over the CUs is then the dispatcher's)
            std::printf("# note: %u B of LDS per block does not pin %u blocks per CU\n", lds, wps);
        float ms[kOps];
        all_ops(out, cus * wps, lds, trips, ms);
        for (int op = 0; op < kOps; ++op) {
            const double ns = (double)ms[op] * 1e6 / ((double)trips * kAcc * kRep);
            std::printf("%-15s %u %.4f %.4f %.3f\n", kNames[op], wps, ms[op], ns, ms[op] / ms[kFmaF32]);
        }
    }
    CHECK(hipFree(out));
    return 0;
}
