// Host check of k_paths' plan over a view's compacted lists (spt_launch_plan.h make_view_plan): the tiers
// cover every live-list index exactly once, the sweep units every constant-list index, the first tier has
// the pixel plan's chunk size, and Cornell 1080p's numbers are what DESIGN.md §3.1e states.
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

// every index of [0, live) in exactly one chunk, every index of [0, constant) in exactly one sweep unit's lane
static void covered_once(const ViewChunkPlan& vp, uint32_t live, uint32_t constant) {
    const ChunkPlan& c = vp.plan;
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
    // sweep unit u, lane l: constant index u * kViewSweep + l when below `constant`
    CHECK((uint64_t)vp.n_sweep * kViewSweep >= constant);
    CHECK(vp.n_sweep == 0 || (uint64_t)(vp.n_sweep - 1u) * kViewSweep < constant);
}

static void view_plan_invariants() {
    const uint32_t Ps[] = {1, 2, 31, 33, 70 * 37, 14400, 259200, 2073600};
    const uint32_t waves[] = {4, 1024, 7168, 8192}, cpws[] = {2, 4}, shifts[] = {0, 2, 5};
    for (uint32_t P : Ps)
        for (uint32_t rw : waves)
            for (uint32_t cpw : cpws)
                for (uint32_t pxs : shifts) {
                    const uint32_t lives[] = {0, 1, P / 3, (uint32_t)(0.38865 * P), P - 1, P};
                    for (uint32_t live : lives) {
                        if (live > P) continue;
                        const ViewChunkPlan vp = make_view_plan(P, live, P - live, rw, cpw, pxs);
                        const ChunkPlan pix = make_chunk_plan(P, rw, cpw, pxs);
                        CHECK(vp.plan.order == nullptr && vp.plan.cost == nullptr);
                        for (int t = 0; t < 3; ++t) CHECK(vp.plan.shift[t] == pix.shift[t]);  // never from the live count
                        if (pxs) CHECK(vp.plan.shift[0] == pxs && vp.plan.n[1] == 0 && vp.plan.n[2] == 0);
                        covered_once(vp, live, P - live);
                        // degenerate views: all sky has no chunk, all live no sweep unit
                        if (live == 0) CHECK(vp.plan.n[0] + vp.plan.n[1] + vp.plan.n[2] == 0 && vp.n_sweep > 0);
                        if (live == P) CHECK(vp.n_sweep == 0);
                        // no small tier has more chunks than the pixel plan's
                        CHECK(vp.plan.n[1] <= (uint64_t)cpw * rw);
                        // the grid counts sweep units as chunks, the key is never a pixel plan's
                        const uint32_t units = vp.plan.n[0] + vp.plan.n[1] + vp.plan.n[2] + vp.n_sweep;
                        CHECK(paths_grid(vp.plan, false, 7, 256, vp.n_sweep) == std::min<uint32_t>((units + 3u) / 4u, 7u * 256u));
                        CHECK(view_order_key(vp.plan, live) != chunk_order_key(pix, P));
                        CHECK(view_order_key(vp.plan, live) != chunk_order_key(vp.plan, live));
                    }
                }
}

// C2: Cornell 1920x1080, 805,896 live pixels, 7 waves/SIMD on 256 CUs, 2 chunks per wave and small tier
static void cornell_1080p() {
    const uint32_t P = 2073600, live = 805896, rw = 7168;
    const ViewChunkPlan vp = make_view_plan(P, live, P - live, rw, 2, 0);
    const ChunkPlan& c = vp.plan;
    CHECK(c.shift[0] == 5 && c.shift[1] == 4 && c.shift[2] == 3);  // from the live count the rule gives 8 pixels
    const uint32_t tail = 5571;  // 2 * 7168 * 805896 / 2073600
    CHECK(c.n[1] == tail && c.n[2] == tail);
    CHECK(c.n[0] == 21006 && c.start[1] == 672192 && c.start[2] == 761328);
    CHECK(((uint64_t)c.n[1] << 4) == 89136 && ((uint64_t)c.n[2] << 3) == 44568);
    CHECK(vp.n_sweep == 19808);
    CHECK(paths_grid(c, false, 7, 256, vp.n_sweep) == 7u * 256u);
    // the pixel plan it replaces: 32-pixel chunks too, its tiers over the image's last pixels
    const ChunkPlan pix = make_chunk_plan(P, rw, 2, 0);
    CHECK(pix.shift[0] == 5 && pix.n[0] == 54048 && pix.n[1] == 14336 && pix.n[2] == 14336);
}

// tests/test_gpu_view_cache.py's 70x37 image: which kernels its cases run on a whole MI355X (7168 resident
// waves) — small chunks under the automatic plan, so the channel-lane kernel; 32-pixel chunks, so the
// pixel-lane kernel, with px_shift = 5; and the same choice over a view's lists as over the pixels
static void test_image_kernels() {
    const uint32_t P = 70 * 37, live = 1007, rw = 7168;
    PassParams p{};
    p.n_prims = 8;
    const ViewChunkPlan a = make_view_plan(P, live, P - live, rw, 2, 0);
    CHECK(a.plan.shift[0] < kMaxChunkShift && a.plan.shift[0] == make_chunk_plan(P, rw, 2, 0).shift[0]);
    CHECK(paths_variant(p, false, a.plan.shift[0]).chan);
    const ViewChunkPlan f = make_view_plan(P, live, P - live, rw, 2, 5);
    CHECK(f.plan.shift[0] == kMaxChunkShift && !paths_variant(p, false, f.plan.shift[0]).chan);
    CHECK(!paths_variant(p, true, a.plan.shift[0]).chan);  // the counting kernels: pixel lanes
}

int main() {
    view_plan_invariants();
    test_image_kernels();
    cornell_1080p();
    if (g_failed) {
        std::printf("%d check(s) failed\n", g_failed);
        return 1;
    }
    std::printf("view plan ok\n");
    return 0;
}
