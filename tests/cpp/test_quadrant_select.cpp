// Host build of spt_device.h's bounce_dir_xy, the tail of bounce_dir_frame: the form that applies the quadrant's
// swap and signs to the two converted floats (kLateQuadrant, k_paths' sampling site under the range bit) against
// the form that selects sin and cos as doubles first. x and y must be the same words, +0 and -0 told apart.
//
// phi = fl(2 pi_f * u2) with u2 = m / 2^32 as random_float forms it from its 32-bit draw m, for m = 0, m = 2^32 - 1
// (the reduction's k = 4), every m that puts phi within kNear floats of a multiple of pi / 2 (found by bisection
// on m: phi is monotone in m), and 2^20 stratified m; sin_t = 0, 2^-16, 2^-12, 0.5, 1 - 2^-24 and 1. Every
// quadrant (and k = 4) must be reached, and both signs of zero must occur among the results.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "spt_device.h"

static uint32_t f2u(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}

static float phi_of(uint64_t m) {
    const float u2 = (float)(uint32_t)m / 4294967295.0f;  // random_float's last line (the divisor is 2^32 as a float)
    return 2.0f * spt::kPiF * u2;
}

int main() {
    const float sin_ts[] = {0.0f, 0x1p-16f, 0x1p-12f, 0.5f, 1.0f - 0x1p-24f, 1.0f};
    constexpr int kNear = 4;  // floats on each side of a multiple of pi / 2
    std::vector<uint32_t> ms = {0u, 0xffffffffu};
    for (int j = 1; j <= 4; ++j) {
        const float target = (float)((double)j * 1.57079632679489661923);
        // the first m whose phi is >= the float kNear below the target, and the last whose phi is <= kNear above
        float lo_f = target, hi_f = target;
        for (int i = 0; i < kNear; ++i) {
            lo_f = std::nextafterf(lo_f, 0.0f);
            hi_f = std::nextafterf(hi_f, 10.0f);
        }
        uint64_t a = 0, b = 1ull << 32;  // smallest m in [a, b] with phi_of(m) >= lo_f (2^32: none)
        while (a < b) {
            const uint64_t mid = (a + b) / 2;
            if (phi_of(mid) >= lo_f) b = mid;
            else a = mid + 1;
        }
        for (uint64_t m = a; m < (1ull << 32) && phi_of(m) <= hi_f; ++m) ms.push_back((uint32_t)m);
    }
    const size_t n_special = ms.size();
    for (uint32_t i = 0; i < (1u << 20); ++i) {  // one m per stratum of 4096, at a position that moves with i
        ms.push_back((i << 12) | ((i * 2654435761u) >> 20));
    }

    unsigned long long bad = 0, n = 0, zeros_pos = 0, zeros_neg = 0;
    unsigned long long quadrant[5] = {0, 0, 0, 0, 0};
    for (const uint32_t m : ms) {
        const float phi = phi_of(m);
        const int k = (int)__builtin_rint((double)phi * 6.36619772367581382433e-01);  // sincos_2pi's reduction
        if (k < 0 || k > 4) {
            std::printf("phi %a: k = %d outside 0..4\n", phi, k);
            return 1;
        }
        ++quadrant[k];
        for (const float sin_t : sin_ts) {
            float x0, y0, x1, y1;
            spt::bounce_dir_xy<false, false>(sin_t, phi, x0, y0);
            spt::bounce_dir_xy<false, true>(sin_t, phi, x1, y1);
            ++n;
            for (const float v : {x0, y0}) {
                zeros_pos += f2u(v) == 0u;
                zeros_neg += f2u(v) == 0x80000000u;
            }
            if (f2u(x0) != f2u(x1) || f2u(y0) != f2u(y1)) {
                if (bad++ < 10)
                    std::printf("m %08x phi %a sin_t %a: x %08x / %08x  y %08x / %08x\n", m, phi, sin_t, f2u(x0), f2u(x1),
                                f2u(y0), f2u(y1));
            }
        }
    }
    std::printf("inputs: %zu around the multiples of pi / 2 and the ends, %zu stratified; x %zu sin_t = %llu pairs\n",
                n_special, ms.size() - n_special, sizeof sin_ts / sizeof sin_ts[0], n);
    std::printf("k = 0..4: %llu %llu %llu %llu %llu; results +0: %llu, -0: %llu\n", quadrant[0], quadrant[1], quadrant[2],
                quadrant[3], quadrant[4], zeros_pos, zeros_neg);
    bool covered = zeros_pos != 0 && zeros_neg != 0;
    for (const unsigned long long q : quadrant) covered = covered && q != 0;
    if (!covered) std::printf("a quadrant or a sign of zero was not reached\n");
    std::printf("mismatches: %llu\n", bad);
    std::printf(bad == 0 && covered ? "PASS\n" : "FAIL\n");
    return bad == 0 && covered ? 0 : 1;
}
