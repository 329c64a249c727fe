// Host check of k_paths' slot split (spt_kernels.h slot_split_shift): for a full chunk of px = 16, 32 and 64 live
// pixels and every slot q < 2^16, the shift-and-mask form gives the frame and the live rank of the general form,
// (div_live(q), q - f * px) with div_live the kernel's high multiply by ceil(2^31 / n_live), and both are the plain
// quotient and remainder. A partial chunk (n_live < px) keeps the multiply: shown here to differ from the shift form,
// so the kernel's n_live == px test is what selects it.
#include <cstdint>
#include <cstdio>

#include "spt_kernels.h"

using namespace spt;

static int g_failed = 0;
#define CHECK(cond)                                                       \
    do {                                                                  \
        if (!(cond)) {                                                    \
            if (++g_failed <= 20) std::printf("line %d: %s\n", __LINE__, #cond); \
        }                                                                 \
    } while (0)

// k_paths' div_live (spt_kernels.hip): __umulhi(s << 1, m_live), m_live = ceil(2^31 / n_live)
static uint32_t div_live(uint32_t s, uint32_t n_live) {
    const uint32_t m_live = (0x80000000u + n_live - 1u) / n_live;
    return (uint32_t)(((uint64_t)(s << 1) * m_live) >> 32);
}

int main() {
    uint64_t checked = 0;
    for (uint32_t pxs : {4u, 5u, 6u}) {
        const uint32_t px = 1u << pxs;
        uint32_t bad = 0;
        for (uint32_t q = 0; q < (1u << 16); ++q) {
            const SlotSplit s = slot_split_shift(q, pxs);
            const uint32_t f = div_live(q, px), r = q - f * px;
            bad += s.f != f || s.r != r || s.f != q / px || s.r != q % px || s.r >= px;
            ++checked;
        }
        CHECK(bad == 0);
    }
    CHECK(kWideShift == 6u && kWidePx == 64u);  // the wide form's first tier, and the largest px
    // the last chunk of a list: n_live < px, where the shift form is NOT the split (the first slot of frame 1 shows it)
    for (uint32_t pxs : {4u, 5u, 6u})
        for (uint32_t n_live = 1; n_live < (1u << pxs); ++n_live) {
            const SlotSplit s = slot_split_shift(n_live, pxs);
            CHECK(div_live(n_live, n_live) == 1u && s.f == 0u && s.r == n_live);
        }
    if (g_failed) {
        std::printf("%d check(s) failed\n", g_failed);
        return 1;
    }
    std::printf("slot split ok: %llu slots\n", (unsigned long long)checked);
    return 0;
}
