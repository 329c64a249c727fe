// Host check of the split of a view's lists into two halves (spt_launch_plan.h make_view_split): the halves
// cover the live and the constant list exactly once, the cuts are chunk- and sweep-aligned, each half's plan
// (make_view_plan with the WHOLE shard's pixels) keeps the unsplit plan's first-tier chunk size and covers
// its half exactly once, and the order keys of half A, half B and the unsplit plan differ pairwise.
#include <cstdio>
#include <vector>

#include "spt_launch_plan.h"

using namespace spt;

static int g_failed = 0;
#define CHECK(cond)                                                       \
    do {                                                                  \
        if (!(cond)) {                                                    \
            if (++g_failed <= 20) std::printf("line %d: %s\n", __LINE__, #cond); \
        }                                                                 \
    } while (0)

// every index of [0, live) in exactly one chunk of the half's plan
static void plan_covers(const ViewChunkPlan& vp, uint32_t live, uint32_t constant) {
    const ChunkPlan& c = vp.plan;
    std::vector<uint8_t> seen(live, 0);
    for (int t = 0; t < 3; ++t)
        for (uint32_t k = 0; k < c.n[t]; ++k) {
            const uint32_t i0 = c.start[t] + (k << c.shift[t]);
            CHECK(i0 < live);
            for (uint32_t j = 0; j < (1u << c.shift[t]) && i0 + j < live; ++j) ++seen[i0 + j];
        }
    uint32_t bad = 0;
    for (uint32_t i = 0; i < live; ++i) bad += seen[i] != 1;
    CHECK(bad == 0);
    CHECK((uint64_t)vp.n_sweep * kViewSweep >= constant);
    CHECK(vp.n_sweep == 0 || (uint64_t)(vp.n_sweep - 1u) * kViewSweep < constant);
}

static void check_split(uint32_t shard_pixels, uint32_t n_live, uint32_t n_const, uint32_t rw, uint32_t cpw) {
    const ViewChunkPlan whole = make_view_plan(shard_pixels, n_live, n_const, rw, cpw, 0);
    const uint32_t px = 1u << whole.plan.shift[0];
    // the library cuts at the largest chunk size (a multiple of every first tier's); the first tier's own too
    for (uint32_t unit : {1u << kMaxChunkShift, px}) {
        const ViewSplit s = make_view_split(n_live, n_const, unit);
        // the halves cover [0, n_live) and [0, n_const) exactly once: contiguous, in order, nothing left
        CHECK(s.live_at[0] == 0 && s.live_at[2] == n_live && s.live_at[1] <= n_live);
        CHECK(s.const_at[0] == 0 && s.const_at[2] == n_const && s.const_at[1] <= n_const);
        // the cuts: chunk- and sweep-aligned, and the multiples nearest the middle
        CHECK(s.live_at[1] % unit == 0 && s.live_at[1] % px == 0);
        CHECK(s.const_at[1] % kViewSweep == 0);
        const int64_t dl = (int64_t)s.live_at[1] - (int64_t)(n_live / 2u);
        CHECK(s.live_at[1] == n_live || (dl <= (int64_t)unit / 2 && -dl <= (int64_t)unit / 2));
        const int64_t dc = (int64_t)s.const_at[1] - (int64_t)(n_const / 2u);
        CHECK(s.const_at[1] == n_const || (dc <= (int64_t)kViewSweep / 2 && -dc <= (int64_t)kViewSweep / 2));
        uint64_t keys[3] = {view_order_key(whole.plan, n_live), 0, 0};
        for (uint32_t h = 0; h < 2u; ++h) {
            const uint32_t live = s.live_at[h + 1] - s.live_at[h], constant = s.const_at[h + 1] - s.const_at[h];
            CHECK(view_half_empty(s, h) == (live == 0 && constant == 0));
            const ViewChunkPlan vp = make_view_plan(shard_pixels, live, constant, rw, cpw, 0);
            for (int t = 0; t < 3; ++t) CHECK(vp.plan.shift[t] == whole.plan.shift[t]);  // never from the half's pixels
            plan_covers(vp, live, constant);
            keys[h + 1] = view_order_key(vp.plan, live, h + 1u);
            // a half's key is never a pixel plan's, and not the same plan's key as the whole view
            CHECK(keys[h + 1] != view_order_key(vp.plan, live));
            CHECK(keys[h + 1] != chunk_order_key(vp.plan, live));
        }
        CHECK(keys[0] != keys[1] && keys[0] != keys[2] && keys[1] != keys[2]);
    }
}

int main() {
    const uint32_t chunk = 1u << kMaxChunkShift;
    const uint32_t lives[] = {0, 1, chunk - 1, chunk, chunk + 1, 2 * chunk, 2 * chunk + 1, 1007, 805896};
    const uint32_t consts[] = {0, 63, 64, 65, 127, 128, 129, 1583, 1267704};
    // a whole MI355X's resident waves, and few enough for a small image to keep 32-pixel chunks
    for (uint32_t rw : {4u, 7168u})
        for (uint32_t live : lives)
            for (uint32_t constant : consts) {
                if (live + constant == 0) continue;
                // chunks per wave and small tier: the pixel plan's 2, and the split launches' 0 (no small tiers)
                for (uint32_t cpw : {2u, 0u}) {
                    check_split(live + constant, live, constant, rw, cpw);
                    check_split(2073600, live, constant, rw, cpw);  // (a view's lists never hold more than the shard)
                }
            }
    // C2: Cornell 1920x1080, 805,896 live and 1,267,704 constant pixels, 7168 resident waves
    const ViewSplit s = make_view_split(805896, 1267704, chunk);
    CHECK(s.live_at[1] == 402944 && s.const_at[1] == 633856);  // 12592 chunks of 32, 9904 sweep units
    const ViewChunkPlan a = make_view_plan(2073600, s.live_at[1], s.const_at[1], 7168, 2, 0);
    const ViewChunkPlan b = make_view_plan(2073600, 805896 - s.live_at[1], 1267704 - s.const_at[1], 7168, 2, 0);
    CHECK(a.plan.shift[0] == 5 && b.plan.shift[0] == 5);  // halving the pixels must not drop C2 to 16-pixel chunks
    CHECK(a.plan.n[1] == 2785 && b.plan.n[1] == 2785);    // each half: half the whole view's 5571 tail chunks per tier
    CHECK(a.n_sweep == 9904 && b.n_sweep == 9904);
    // ... and what the library launches: no small tiers (0 chunks per wave), the first tier's leftover records
    // in the last tier's 8-pixel chunks
    const ViewChunkPlan a0 = make_view_plan(2073600, s.live_at[1], s.const_at[1], 7168, 0, 0);
    const ViewChunkPlan b0 = make_view_plan(2073600, 805896 - s.live_at[1], 1267704 - s.const_at[1], 7168, 0, 0);
    CHECK(a0.plan.shift[0] == 5 && a0.plan.n[0] == 12592 && a0.plan.n[1] == 0 && a0.plan.n[2] == 0);
    CHECK(b0.plan.shift[0] == 5 && b0.plan.n[0] == 12592 && b0.plan.n[1] == 0 && b0.plan.n[2] == 1);  // 402,952 = 12592 * 32 + 8
    // degenerate halves: fewer than half a unit goes to B whole, and an empty half is recognisable
    const ViewSplit tiny = make_view_split(1, 0, chunk);
    CHECK(view_half_empty(tiny, 0) && !view_half_empty(tiny, 1));
    const ViewSplit sky = make_view_split(0, 64, chunk);
    CHECK(!view_half_empty(sky, 0) && view_half_empty(sky, 1) && sky.const_at[1] == 64);
    // split or whole is decided for a call, from its largest launch: a short last launch of a long call gets the
    // call's answer (C2's 805,896 live pixels: 1024 frames and a remainder of 1..20 would flip a per-launch rule)
    for (uint32_t frames : {1025u, 1044u, 2048u + 7u, 1024u, 64u, 21u})
        CHECK(split_call_wanted(0, 805896, frames, 1024));
    CHECK(!split_call_wanted(0, 805896, 20, 1024));  // 16.1 M live-pixel frames, below 2^24
    CHECK(split_call_wanted(0, 358000, 64, 1024) && !split_call_wanted(0, 50000, 64, 1024));  // 720p, 480x270
    CHECK(!split_call_wanted(0, 2400, 64, 1024) && !split_call_wanted(0, 2400, 5000, 1024));  // 96x64
    CHECK(split_call_wanted(0, 22400, 1032, 1024) && !split_call_wanted(0, 22400, 8, 1024));  // 320x180: the GPU test's calls
    CHECK(split_call_wanted(1, 1, 4, 1024) && !split_call_wanted(-1, 805896, 1024, 1024));    // the knob forced
    if (g_failed) {
        std::printf("%d check(s) failed\n", g_failed);
        return 1;
    }
    std::printf("split plan ok\n");
    return 0;
}
