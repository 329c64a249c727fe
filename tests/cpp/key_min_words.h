// The closest-hit keys that tests/cpp/test_key_min.hip (device) and tests/cpp/test_key_min_host.cpp (host) run
// spt_device.h key_min over: a key is (high word << 32) | low word, the high word a t's float bits, the low word a
// primitive's original index. Included after spt_device.h.
#pragma once

namespace key_min_words {

constexpr uint32_t kTNearBits = 0x3a83126fu;  // bits(spt::kTNear = 0.001f)
static_assert(__builtin_bit_cast(uint32_t, spt::kTNear) == kTNearBits, "kTNear's bits");

constexpr uint32_t kNHigh = 9, kNLow = 6;
// High words: the smallest, the largest denormal double's and the smallest normal double's (a tiny shadow-ray
// smax), kTNear and its two neighbours, 1.0f, the largest finite float, +inf (a miss).
__host__ __device__ inline uint32_t high_word(uint32_t i) {
    constexpr uint32_t w[kNHigh] = {0x00000001u, 0x000fffffu, 0x00100000u, kTNearBits - 1u, kTNearBits,
                                    kTNearBits + 1u, 0x3f800000u, 0x7f7fffffu, 0x7f800000u};
    return w[i];
}
// Low words: the ends of the index range, a small index, either side of the word's top bit, and kMiss.
__host__ __device__ inline uint32_t low_word(uint32_t i) {
    constexpr uint32_t w[kNLow] = {0u, 1u, 31u, 0x7fffffffu, 0x80000000u, 0xffffffffu};
    return w[i];
}
constexpr uint32_t kNKeys = kNHigh * kNLow;
constexpr uint32_t kNPairs = kNKeys * kNKeys;  // every ordered pair: both operand orders, equal keys included
constexpr uint32_t kNRandom = 1u << 22;        // random pairs, high words in [kTNearBits, 0x7f800000]

__host__ __device__ inline uint64_t set_key(uint32_t k) {  // k < kNKeys
    return ((uint64_t)high_word(k / kNLow) << 32) | low_word(k % kNLow);
}

__host__ __device__ inline uint32_t hash32(uint32_t x) {  // (the PCG output function over an LCG step)
    x = x * 747796405u + 2891336453u;
    x = ((x >> ((x >> 28) + 4u)) ^ x) * 277803737u;
    return (x >> 22) ^ x;
}
// Random pair i: two keys with high words in [kTNearBits, 0x7f800000]; one pair in eight shares its high word (a
// tie on t, decided by the index), one in sixty-four is a pair of equal keys.
__host__ __device__ inline void random_pair(uint32_t i, uint64_t& a, uint64_t& b) {
    constexpr uint32_t kSpan = 0x7f800000u - kTNearBits + 1u;
    const uint32_t ha = kTNearBits + hash32(4u * i + 0u) % kSpan, la = hash32(4u * i + 1u);
    uint32_t hb = kTNearBits + hash32(4u * i + 2u) % kSpan, lb = hash32(4u * i + 3u);
    if ((i & 7u) == 0u) hb = ha;
    if ((i & 63u) == 0u) lb = la;
    a = ((uint64_t)ha << 32) | la;
    b = ((uint64_t)hb << 32) | lb;
}

// The reference: the keys' order as unsigned integers, word by word.
__host__ __device__ inline uint64_t min_by_words(uint64_t a, uint64_t b) {
    const uint32_t ha = (uint32_t)(a >> 32), hb = (uint32_t)(b >> 32), la = (uint32_t)a, lb = (uint32_t)b;
    const bool a_first = ha != hb ? ha < hb : la <= lb;
    return a_first ? a : b;
}

}  // namespace key_min_words
