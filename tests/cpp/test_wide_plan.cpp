// Host check of the wide form's plans (spt_launch_plan.h make_view_plan / make_view_split with their trailing
// parameters, wide_call / wide_launch) and of the bounds k_paths' wide chunks rely on: the live-rank division,
// the ring's lap byte under the 512-frame cap, the uint16 chunk cost and the step bound.
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

static bool same_plan(const ChunkPlan& a, const ChunkPlan& b) {
    for (int t = 0; t < 3; ++t)
        if (a.n[t] != b.n[t] || a.start[t] != b.start[t] || a.shift[t] != b.shift[t]) return false;
    return a.order == b.order && a.cost == b.cost;
}

// every index of [0, live) in exactly one chunk; no chunk starts at or past `live`
static void covered_once(const ChunkPlan& c, uint32_t live) {
    std::vector<uint8_t> seen(live, 0);
    for (int t = 0; t < 3; ++t)
        for (uint32_t k = 0; k < c.n[t]; ++k) {
            const uint32_t i0 = c.start[t] + (k << c.shift[t]);
            CHECK(i0 < live);  // k_paths: npx = min(px, n_live - pix0) needs pix0 < n_live
            for (uint32_t j = 0; j < (1u << c.shift[t]) && i0 + j < live; ++j) ++seen[i0 + j];
        }
    uint32_t bad = 0;
    for (uint32_t i = 0; i < live; ++i) bad += seen[i] != 1;
    CHECK(bad == 0);
}

// the trailing parameters' defaults give the plans of before, with C2's numbers
static void defaults_are_todays() {
    const uint32_t P = 2073600, live = 805896, rw = 7168;
    const ViewChunkPlan d = make_view_plan(P, live, P - live, rw, 2, 0), n = make_view_plan(P, live, P - live, rw, 2, 0, false);
    CHECK(same_plan(d.plan, n.plan) && d.n_sweep == n.n_sweep);
    CHECK(d.plan.shift[0] == 5 && d.plan.n[0] == 21006 && d.plan.n[1] == 5571 && d.plan.n[2] == 5571);
    CHECK(d.plan.start[1] == 672192 && d.plan.start[2] == 761328 && d.n_sweep == 19808);
    const ViewSplit s = make_view_split(live, P - live), s32 = make_view_split(live, P - live, 32u);
    CHECK(s.live_at[1] == s32.live_at[1] && s.const_at[1] == s32.const_at[1]);
    CHECK(s.live_at[1] == 402944 && s.live_at[1] % 32u == 0 && s.const_at[1] % kViewSweep == 0);
    // a forced chunk size is a forced chunk size: `wide` changes nothing then
    const ViewChunkPlan f = make_view_plan(P, live, P - live, rw, 2, 5), fw = make_view_plan(P, live, P - live, rw, 2, 5, true);
    CHECK(same_plan(f.plan, fw.plan));
    PassParams p{};
    p.n_prims = 8;
    p.shard_count = 1;
    CHECK(!paths_variant(p, false, 5).wide && paths_variant(p, false, kWideShift, true).wide);
    CHECK(!paths_variant(p, false, kWideShift, true).chan && paths_variant(p, true, kWideShift, true).wide);
}

// C2's wide plans: whole, and the halves of the split (no small tiers: chunks_per_wave 0 under the split)
static void cornell_1080p_wide() {
    const uint32_t P = 2073600, live = 805896, rw = 7168;
    const ViewChunkPlan w = make_view_plan(P, live, P - live, rw, 2, 0, true);
    CHECK(w.plan.shift[0] == 6 && w.plan.shift[1] == 5 && w.plan.shift[2] == 4);
    // the same 5571 chunks per small tier, of twice the pixels; the last tier also takes the 56 records the
    // first tier's rounding to 64 leaves
    CHECK(w.plan.n[1] == 5571 && w.plan.n[2] == 5571 + 4 && w.plan.start[2] - w.plan.start[1] == 5571u * 32u);
    CHECK(w.plan.n[0] == (live - 5571u * 48u) / 64u);
    covered_once(w.plan, live);
    const ViewSplit s = make_view_split(live, P - live, kWidePx);
    CHECK(s.live_at[1] % kWidePx == 0 && s.live_at[1] == 402944);
    for (uint32_t h = 0; h < 2; ++h) {
        const uint32_t n = s.live_at[h + 1] - s.live_at[h];
        const ViewChunkPlan v = make_view_plan(P, n, s.const_at[h + 1] - s.const_at[h], rw, 0, 0, true);
        CHECK(v.plan.n[0] == n / 64u && v.plan.n[1] == 0 && v.plan.n[2] == (n % 64u + 15u) / 16u);
        covered_once(v.plan, n);
    }
}

static void wide_invariants() {
    const uint32_t Ps[] = {1, 2, 63, 65, 24 * 16, 70 * 37, 14400, 259200, 2073600};
    const uint32_t waves[] = {4, 1024, 7168}, cpws[] = {0, 2, 4};
    for (uint32_t P : Ps)
        for (uint32_t rw : waves)
            for (uint32_t cpw : cpws) {
                const uint32_t lives[] = {0, 1, 31, 63, 64, 65, 127, P / 3, (uint32_t)(0.38865 * P), P - 1, P};
                for (uint32_t live : lives) {
                    if (live > P) continue;
                    const ViewChunkPlan vp = make_view_plan(P, live, P - live, rw, cpw, 0, true);
                    const ChunkPlan& c = vp.plan;
                    CHECK(c.shift[0] == kWideShift && c.shift[1] <= kMaxChunkShift && c.shift[2] <= kMaxChunkShift);
                    covered_once(c, live);
                    CHECK(c.start[1] % kWidePx == 0);
                    // a list of at least four chunks keeps a first tier
                    if (live >= 4u * kWidePx) CHECK(c.n[0] >= 1u);
                    if (live == 0) CHECK(c.n[0] + c.n[1] + c.n[2] == 0);
                    CHECK(view_order_key(c, live) != view_order_key(make_view_plan(P, live, P - live, rw, cpw, 0).plan, live));
                    // the split: the cut on a multiple of 64, no chunk and no sweep unit across it, empty and tiny halves
                    const ViewSplit s = make_view_split(live, P - live, kWidePx);
                    CHECK(s.live_at[0] == 0 && s.live_at[2] == live && s.live_at[1] <= live);
                    CHECK(s.live_at[1] % kWidePx == 0 || s.live_at[1] == live);
                    CHECK(s.const_at[1] % kViewSweep == 0 || s.const_at[1] == P - live);
                    if (live < kWidePx / 2u) CHECK(s.live_at[1] == 0);  // shorter than half a chunk: to B whole
                    for (uint32_t h = 0; h < 2; ++h) {
                        const uint32_t n = s.live_at[h + 1] - s.live_at[h];
                        if (view_half_empty(s, h)) CHECK(n == 0);
                        // (a half's plan is laid over its own part of the list, so no chunk reaches the other's)
                        covered_once(make_view_plan(P, n, s.const_at[h + 1] - s.const_at[h], rw, 0, 0, true).plan, n);
                        covered_once(make_view_plan(P, n, s.const_at[h + 1] - s.const_at[h], rw, 0, 0, false).plan, n);
                    }
                }
            }
}

// small images forced wide, as tests/test_gpu_wide_chunks.py runs them (a 70x37 image with 1007 live records):
// 64-pixel chunks, both small tiers and a partial chunk; one chunk of a 24x16 image; none below 64 records
static void test_image_plans() {
    const ViewChunkPlan a = make_view_plan(70 * 37, 1007, 70 * 37 - 1007, 7168, 2, 0, true);
    CHECK(a.plan.n[0] == 8 && a.plan.n[1] == 7 && a.plan.start[1] == 512 && a.plan.start[2] == 736 && a.plan.n[2] == 17);
    const ViewChunkPlan b = make_view_plan(24 * 16, 150, 24 * 16 - 150, 7168, 2, 0, true);
    CHECK(b.plan.n[0] >= 1);
    const ViewChunkPlan t = make_view_plan(77, 30, 47, 7168, 2, 0, true);
    CHECK(t.plan.n[0] == 0 && t.plan.n[1] + t.plan.n[2] >= 1);
}

// the knob, the automatic rule and what is eligible
static void wide_rule() {
    PassParams p{};
    p.n_prims = 8;
    p.shard_count = 1;
    CHECK(wide_eligible(p));
    PassParams q = p;
    q.shard_count = 2;
    CHECK(!wide_eligible(q));
    q = p;
    q.nee.n_emit = 1;
    CHECK(!wide_eligible(q));
    q = p;
    q.px_shift = 5;
    CHECK(!wide_eligible(q));
    q = p;
    q.cam_mode = kCamJitter;
    CHECK(!wide_eligible(q));
    q = p;
    q.bsdf = 1;
    CHECK(!wide_eligible(q));
    CHECK(wide_call(-1, true, true, 805896, 64) == 0 && wide_call(1, false, true, 805896, 64) == 0);
    CHECK(wide_call(1, true, false, 10, 1) == 2);
    CHECK(wide_call(0, true, true, 805896, 64) == 1);    // C2: 51.6 M live-pixel frames
    CHECK(wide_call(0, true, true, 805896, 4) == 1);     // 3.2 M: the smallest launch measured
    CHECK(wide_call(0, true, true, 805896, 3) == 0);     // 2.4 M: below the threshold
    CHECK(wide_call(0, true, false, 357935, 64) == 0);   // 720p: its plan starts with 16-pixel chunks
    CHECK(wide_call(0, true, true, 1007, 100000) == 0);  // frames count up to a launch's 512
    CHECK(wide_call(0, true, true, 6144, 512) == 1 && wide_call(0, true, true, 6143, 512) == 0);
    CHECK(wide_launch(2, 0) && wide_launch(1, kMaxChunkShift) && !wide_launch(1, kMaxChunkShift - 1u) && !wide_launch(0, kMaxChunkShift));
    // an MI355X: 256 CUs; 1080p and 4K start with 32-pixel chunks, 720p and the 1/8 shard of 1080p do not
    CHECK(wide_first_tier(2073600, 256) && wide_first_tier(3840 * 2160, 256) && !wide_first_tier(921600, 256) && !wide_first_tier(259200, 256));
    CHECK(wide_first_tier(2073600, 256) == (make_chunk_plan(2073600, 7168, 2, 0).shift[0] == kMaxChunkShift));
    CHECK(!wide_possible(-1, 2073600, 1, 256) && !wide_possible(0, 2073600, 8, 256) && wide_possible(0, 2073600, 1, 256));
    CHECK(wide_possible(1, 100, 1, 256) && !wide_possible(0, 70 * 37, 1, 256) && !wide_possible(0, 921600, 1, 256));
}

// k_paths' div_live: floor(s / n) as (2s * ceil(2^31 / n)) >> 32, for every n <= 64 and s <= 2^16
static void div_live_exact() {
    uint32_t bad = 0;
    for (uint32_t n = 1; n <= kWidePx; ++n) {
        const uint32_t m = (0x80000000u + n - 1u) / n;
        for (uint32_t s = 0; s <= (1u << 16); ++s) bad += (uint32_t)(((uint64_t)(s << 1) * m) >> 32) != s / n;
    }
    CHECK(bad == 0);
}

// The ring's done byte: slot q's lap q / 256 + 1 must fit a byte lane of the 4-slot compare (want = lap *
// 0x01010101), so lap <= 255, and differ from the byte the lap before left (lap - 1, or 0 at the chunk's start).
// Rule chosen: wide launches take at most kWideMaxFrames frames; a narrow one 1024 frames of <= 32 pixels.
static void lap_byte() {
    const uint32_t kRing = 256u;
    CHECK((uint64_t)kWideMaxFrames * kWidePx == 1024ull * (1u << kMaxChunkShift));  // the slots of a narrow chunk at most
    const uint32_t last = kWideMaxFrames * kWidePx - 1u;
    CHECK(last / kRing + 1u == 128u);
    for (uint32_t q = 0; q <= last; q += 61u) {
        const uint32_t lap = q / kRing + 1u;
        CHECK(lap <= 255u && (uint8_t)lap == lap && (uint8_t)lap != (uint8_t)(lap - 1u));
        CHECK(((lap * 0x01010101u) >> 24) == lap);  // no carry between the byte lanes
    }
    CHECK((1024u * kWidePx - 1u) / kRing + 1u == 256u);  // what the cap excludes: 1024 frames x 64 pixels wraps the byte
    // the step bound and the recorded cost: (slots + 64) * (bounces + 2) + frames + 4096 in 32 bits for the most slots
    const uint64_t bound = ((uint64_t)kWideMaxFrames * kWidePx + 64u) * (kMaxBounces + 2u) + kWideMaxFrames + 4096u;
    CHECK(bound < (1ull << 32));
}

int main() {
    defaults_are_todays();
    cornell_1080p_wide();
    wide_invariants();
    test_image_plans();
    wide_rule();
    div_live_exact();
    lap_byte();
    if (g_failed) {
        std::printf("%d check(s) failed\n", g_failed);
        return 1;
    }
    std::printf("wide plan ok\n");
    return 0;
}
