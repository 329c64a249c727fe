// GPU check of spt_device.h key_min (the closest-hit keys' minimum as one v_min_f64) against the integer minimum,
// bit for bit:
//   - every ordered pair of the keys made from key_min_words.h's high and low words (both operand orders, equal high
//     words and equal keys included): denormal doubles' high words, kTNear and its neighbours, 1.0f, the largest
//     finite float, +inf; indices at both ends, either side of the word's top bit, kMiss;
//   - 2^22 random pairs with high words in [bits(kTNear), 0x7f800000], each in both operand orders.
// One thread per pair; the integer minimum is taken twice, as a < b ? a : b and word by word (min_by_words).
#include <hip/hip_runtime.h>

#include <cstdio>

#include "spt_device.h"

#include "key_min_words.h"

using namespace spt;
using namespace key_min_words;

namespace {

enum { kBadSet, kBadRandom, kTookFirst, kTookSecond, kCounters };

__global__ __launch_bounds__(256) void k_check(uint32_t n, unsigned long long* ctr, uint32_t* first_bad) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    uint64_t a, b;
    const bool set = i < kNPairs;
    if (set) {
        a = set_key(i / kNKeys);
        b = set_key(i % kNKeys);
    } else {
        random_pair(i - kNPairs, a, b);
    }
    const uint64_t want = a < b ? a : b;
    bool bad = want != min_by_words(a, b);
    bad = bad || key_min(a, b) != want || key_min(b, a) != want;
    if (bad) {
        atomicAdd(&ctr[set ? kBadSet : kBadRandom], 1ull);
        atomicMin(first_bad, i);
    }
    atomicAdd(&ctr[want == a ? kTookFirst : kTookSecond], 1ull);  // (equal keys count as the first)
}

bool ck(hipError_t e, const char* what) {
    if (e == hipSuccess) return true;
    std::printf("HIP error: %s: %s\n", what, hipGetErrorString(e));
    return false;
}

}  // namespace

int main() {
    unsigned long long* d_ctr = nullptr;
    uint32_t* d_first = nullptr;
    unsigned long long ctr[kCounters] = {};
    uint32_t first = 0xffffffffu;
    if (!ck(hipMalloc((void**)&d_ctr, sizeof ctr), "hipMalloc") || !ck(hipMalloc((void**)&d_first, 4), "hipMalloc") ||
        !ck(hipMemset(d_ctr, 0, sizeof ctr), "hipMemset") || !ck(hipMemcpy(d_first, &first, 4, hipMemcpyHostToDevice), "hipMemcpy"))
        return 1;
    constexpr uint32_t n = kNPairs + kNRandom;
    hipLaunchKernelGGL(k_check, dim3((n + 255u) / 256u), dim3(256), 0, 0, n, d_ctr, d_first);
    if (!ck(hipGetLastError(), "k_check") || !ck(hipDeviceSynchronize(), "k_check") ||
        !ck(hipMemcpy(ctr, d_ctr, sizeof ctr, hipMemcpyDeviceToHost), "hipMemcpy") ||
        !ck(hipMemcpy(&first, d_first, 4, hipMemcpyDeviceToHost), "hipMemcpy"))
        return 1;
    (void)hipFree(d_ctr);
    (void)hipFree(d_first);
    std::printf("key_min: %u set pairs (%u keys), %u random pairs; mismatches %llu (set) %llu (random); the minimum was the "
                "first operand %llu times, the second %llu\n", kNPairs, kNKeys, kNRandom, ctr[kBadSet], ctr[kBadRandom],
                ctr[kTookFirst], ctr[kTookSecond]);
    if (first != 0xffffffffu) std::printf("first bad pair: %u\n", first);
    // both outcomes ran, and every pair was counted
    const bool both = ctr[kTookFirst] > n / 4u && ctr[kTookSecond] > n / 4u && ctr[kTookFirst] + ctr[kTookSecond] == n;
    const bool ok = !ctr[kBadSet] && !ctr[kBadRandom] && both;
    if (!both) std::printf("the counts of the two outcomes are outside what the inputs are built for\n");
    std::printf("%s\n", ok ? "PASS" : "FAIL");
    return ok ? 0 : 1;
}
