// Host check of spt_device.h key_min: the CPU build's branch (the integer minimum) over the pairs that
// tests/cpp/test_key_min.hip runs on the device, against the keys' order word by word (key_min_words.h
// min_by_words). It also checks, on the same pairs, the fact the device form rests on: the two keys read as doubles
// are positive and finite, and they order as the integers do (denormal doubles included).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>

#include "spt_device.h"

#include "key_min_words.h"

using namespace key_min_words;

int main() {
    unsigned long long bad_min = 0, bad_order = 0, bad_domain = 0, first = 0, second = 0, denormal = 0;
    auto check = [&](uint64_t a, uint64_t b) {
        const uint64_t want = min_by_words(a, b);
        if (spt::key_min(a, b) != want || spt::key_min(b, a) != want) ++bad_min;
        double da, db;
        std::memcpy(&da, &a, 8);
        std::memcpy(&db, &b, 8);
        if (!(da > 0.0 && std::isfinite(da) && db > 0.0 && std::isfinite(db))) ++bad_domain;
        if ((da < db) != (a < b) || (da == db) != (a == b)) ++bad_order;
        denormal += std::fpclassify(da) == FP_SUBNORMAL;
        ++(want == a ? first : second);
    };
    for (uint32_t i = 0; i < kNPairs; ++i) check(set_key(i / kNKeys), set_key(i % kNKeys));
    for (uint32_t i = 0; i < kNRandom; ++i) {
        uint64_t a, b;
        random_pair(i, a, b);
        check(a, b);
    }
    const unsigned long long n = (unsigned long long)kNPairs + kNRandom;
    std::printf("key_min (host): %u set pairs (%u keys), %u random pairs; mismatches: %llu; pairs outside the positive finite "
                "doubles: %llu; pairs whose doubles order otherwise: %llu; denormal first operands %llu; the minimum was the "
                "first operand %llu times, the second %llu\n", kNPairs, kNKeys, kNRandom, bad_min, bad_domain, bad_order,
                denormal, first, second);
    const bool cover = first > n / 4u && second > n / 4u && denormal >= 2ull * kNLow * kNKeys;
    const bool ok = !bad_min && !bad_domain && !bad_order && cover;
    if (!cover) std::printf("the inputs do not cover what they are built for\n");
    std::printf("%s\n", ok ? "PASS" : "FAIL");
    return ok ? 0 : 1;
}
