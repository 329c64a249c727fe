// Host check of the persistent kernels' launch planning (spt_launch_plan.h): the chunk plan of k_paths,
// which instantiation of k_paths / k_frame a scene runs and its run-time compiled kind, k_frame's grid,
// and the name expressions of the run-time compiled kinds (spt_jit.h). Every variant computes the same
// image, so only a check like this one sees a wrong choice.
#include <cstdio>
#include <cstring>
#include <string>

#include "spt_launch_plan.h"

using namespace spt;

static int g_failed = 0;
#define CHECK(cond)                                                       \
    do {                                                                  \
        if (!(cond)) {                                                    \
            if (++g_failed <= 20) std::printf("line %d: %s\n", __LINE__, #cond); \
        }                                                                 \
    } while (0)

static bool tiers_are(const ChunkPlan& c, const uint32_t (&shift)[3], const uint32_t (&n)[3], const uint32_t (&start)[3]) {
    return !std::memcmp(c.shift, shift, sizeof shift) && !std::memcmp(c.n, n, sizeof n) && !std::memcmp(c.start, start, sizeof start);
}

static void chunk_plan_invariants() {
    const uint32_t Ps[] = {1, 2, 31, 32, 33, 1000, 1023, 14400, 259200, 2073600, 8294400};
    const uint32_t waves[] = {4, 1024, 7168, 8192}, cpws[] = {2, 4}, shifts[] = {0, 2, 3, 5};
    for (uint32_t P : Ps)
        for (uint32_t rw : waves)
            for (uint32_t cpw : cpws)
                for (uint32_t pxs : shifts) {
                    const ChunkPlan c = make_chunk_plan(P, rw, cpw, pxs);
                    CHECK(c.order == nullptr && c.cost == nullptr);
                    // the tiers tile [0, P) in order; only the last chunk may overhang, by less than its size
                    uint64_t at = 0;
                    int last = -1;
                    for (int t = 0; t < 3; ++t) {
                        CHECK(c.shift[t] >= kMinChunkShift && c.shift[t] <= kMaxChunkShift);
                        if (t) CHECK(c.shift[t] <= c.shift[t - 1]);
                        if (!c.n[t]) continue;
                        CHECK(c.start[t] == at);
                        at += (uint64_t)c.n[t] << c.shift[t];
                        last = t;
                    }
                    CHECK(last >= 0 && at >= P && at - P < (1ull << c.shift[last]));
                    for (int t = 0; t < last; ++t) CHECK(c.start[t] + ((uint64_t)c.n[t] << c.shift[t]) <= P);
                    if (pxs) {
                        CHECK(c.shift[0] == pxs && c.n[1] == 0 && c.n[2] == 0);
                    } else {
                        uint32_t want = kMinChunkShift;
                        for (uint32_t s = kMaxChunkShift; s > kMinChunkShift; --s)
                            if (((uint64_t)P >> s) >= 8ull * rw) {
                                want = s;
                                break;
                            }
                        CHECK(c.shift[0] == want);
                    }
                }
}

static void chunk_plan_values() {
    static_assert(kMinChunkShift == 0 && kMaxChunkShift == 5, "the values below are for these bounds");
    CHECK(tiers_are(make_chunk_plan(2073600, 7168, 2, 0), {5, 4, 3}, {54048, 14336, 14336}, {0, 1729536, 1958912}));
    CHECK(tiers_are(make_chunk_plan(2073600, 8192, 4, 0), {4, 3, 2}, {105024, 32768, 32768}, {0, 1680384, 1942528}));
    CHECK(tiers_are(make_chunk_plan(259200, 7168, 2, 0), {2, 1, 0}, {54048, 14336, 14336}, {0, 216192, 244864}));
    CHECK(tiers_are(make_chunk_plan(1023, 4, 2, 0), {4, 3, 2}, {57, 8, 12}, {0, 912, 976}));
    ChunkPlan c = make_chunk_plan(14400, 7168, 2, 0);
    CHECK(c.shift[0] == 0 && c.n[0] == 14400 && c.n[1] == 0 && c.n[2] == 0);
    c = make_chunk_plan(2073600, 7168, 2, 3);
    CHECK(c.shift[0] == 3 && c.n[0] == 259200 && c.n[1] == 0 && c.n[2] == 0);
    CHECK(chunk_order_key(make_chunk_plan(2073600, 7168, 2, 0), 2073600) == (54048ull << 37 | 2073600ull << 5 | 5));
    // the grid: one block per 4 chunks at most, else all resident blocks (BVH: at most kMaxResidentWaves per CU)
    CHECK(paths_grid(make_chunk_plan(2073600, 7168, 2, 0), false, 7, 256) == 7 * 256);
    CHECK(paths_grid(make_chunk_plan(1023, 4, 2, 0), false, 7, 256) == (57 + 8 + 12 + 3) / 4);
    CHECK(paths_grid(make_chunk_plan(2073600, 8192, 2, 0), true, 9, 256) == 8 * 256);
    CHECK(resident_waves(7, 256) == 7168);
}

static const float4 kSome[1] = {};
static uint32_t g_rgba[1];
// a flat scene of 20 primitives, or a BVH scene of `bvh_prims`
static PassParams scene(uint32_t bvh_prims, uint32_t n_emit = 0, uint32_t spheres = 0, bool env = false) {
    PassParams p{};
    p.prims = kSome;
    p.mats = kSome;
    p.nodes = bvh_prims ? kSome : nullptr;
    p.n_prims = bvh_prims ? bvh_prims : 20;
    p.n_mats = 4;
    p.n_dev_nodes = bvh_prims ? (bvh_prims + 2) / 3 : 0;
    p.stack_need = bvh_prims ? 8 : 0;
    p.env = env ? kSome : nullptr;
    p.nee = NeeParams{n_emit ? kSome : nullptr, n_emit, spheres};
    p.jit_shape = bvh_prims ? 0 : flat_shape_key(0, 20);
    return p;
}
static bool same(const PathsVariant& a, const PathsVariant& b) {
    return a.stats == b.stats && a.bvh == b.bvh && a.env == b.env && a.simd_waves == b.simd_waves && a.chan == b.chan && a.nee == b.nee;
}
static bool same(const FrameVariant& a, const FrameVariant& b) {
    return a.stats == b.stats && a.bvh == b.bvh && a.env == b.env && a.small == b.small && a.nee == b.nee && a.rgba == b.rgba;
}
static bool same(JitKind a, JitKind b) { return a.kind == b.kind && (a.kind < 0 || a.env == b.env); }

static void selectors() {
    const uint64_t shape = flat_shape_key(0, 20);
    // flat, gradient sky / environment map, statistics off and on
    CHECK(same(paths_variant(scene(0), false, 5), PathsVariant{false, false, 0, 0, false, 0}));
    CHECK(same(paths_variant(scene(0, 0, 0, true), false, 5), PathsVariant{false, false, 1, 0, false, 0}));
    CHECK(same(paths_variant(scene(0), true, 5), PathsVariant{true, false, 0, 0, false, 0}));
    // chan: a flat scene whose first shift is below kMaxChunkShift, statistics and NEE off
    CHECK(same(paths_variant(scene(0), false, 4), PathsVariant{false, false, 0, 0, true, 0}));
    CHECK(same(paths_variant(scene(0, 0, 0, true), false, 0), PathsVariant{false, false, 1, 0, true, 0}));
    CHECK(!paths_variant(scene(0), true, 4).chan);
    CHECK(!paths_variant(scene(0, 3, 1), false, 4).chan);
    CHECK(!paths_variant(scene(1000), false, 4).chan);
    // BVH: 8 waves up to kBvhSmall primitives, without statistics and NEE
    CHECK(same(paths_variant(scene(kBvhSmall), false, 5), PathsVariant{false, true, 0, kBvhSmallWaves, false, 0}));
    CHECK(same(paths_variant(scene(kBvhSmall + 1), false, 5), PathsVariant{false, true, 0, 0, false, 0}));
    CHECK(same(paths_variant(scene(1000, 0, 0, true), true, 5), PathsVariant{true, true, 1, 0, false, 0}));
    CHECK(paths_variant(scene(1000, 2, 0), false, 5).simd_waves == 0);
    // NEE: env 2; kNeeNoSpheres only for a BVH scene without a sphere emitter; a flat scene is always kNeeAll
    CHECK(same(paths_variant(scene(1000, 2, 0, true), false, 5), PathsVariant{false, true, 2, 0, false, kNeeNoSpheres}));
    CHECK(same(paths_variant(scene(1000, 2, 1), true, 5), PathsVariant{true, true, 2, 0, false, kNeeAll}));
    CHECK(same(paths_variant(scene(0, 2, 0), false, 3), PathsVariant{false, false, 2, 0, false, kNeeAll}));
    CHECK(same(paths_variant(scene(0, 2, 2), true, 5), PathsVariant{true, false, 2, 0, false, kNeeAll}));
    CHECK(same(frame_variant(scene(1000, 2, 0), false), FrameVariant{false, true, 2, false, kNeeNoSpheres, false}));
    CHECK(same(frame_variant(scene(1000, 2, 1), true), FrameVariant{true, true, 2, false, kNeeAll, false}));
    CHECK(same(frame_variant(scene(0, 2, 0, true), false), FrameVariant{false, false, 2, false, kNeeAll, false}));
    // k_frame: statistics, and the fused resolve forcing them off
    CHECK(same(frame_variant(scene(0), false), FrameVariant{false, false, 0, false, 0, false}));
    CHECK(same(frame_variant(scene(0, 0, 0, true), true), FrameVariant{true, false, 1, false, 0, false}));
    CHECK(same(frame_variant(scene(1000), true), FrameVariant{true, true, 0, false, 0, false}));
    PassParams r = scene(0);
    r.rgba = g_rgba;
    CHECK(same(frame_variant(r, true), FrameVariant{false, false, 0, false, 0, true}));
    r = scene(0, 2, 0);
    r.rgba = g_rgba;
    CHECK(same(frame_variant(r, true), FrameVariant{false, false, 2, false, kNeeAll, true}));
    // small: frame_small_scene at its four boundaries, and off with statistics or NEE
    PassParams s = scene(kFrameTopPrims);
    s.n_dev_nodes = kFrameTopNodes;
    s.n_mats = 0;
    s.stack_need = kFrameLdsStackMax;
    CHECK(frame_small_scene(s, false));
    CHECK(same(frame_variant(s, false), FrameVariant{false, true, 0, true, 0, false}));
    CHECK(same(frame_variant(s, true), FrameVariant{true, true, 0, false, 0, false}));
    r = s;
    r.rgba = g_rgba;
    CHECK(same(frame_variant(r, true), FrameVariant{false, true, 0, true, 0, true}));  // (statistics are off first)
    r = s;
    r.n_dev_nodes = kFrameTopNodes + 1;
    CHECK(!frame_variant(r, false).small);
    r = s;
    r.n_prims = kFrameTopPrims + 1;
    CHECK(!frame_variant(r, false).small);
    r = s;
    r.n_mats = 1;  // 4 * prims + 2 * mats float4s no longer fit the LDS records
    CHECK(!frame_variant(r, false).small);
    r.n_prims = kFrameTopPrims - 1;
    r.n_mats = 2;
    CHECK(frame_variant(r, false).small);
    r = s;
    r.stack_need = kFrameLdsStackMax + 1;
    CHECK(!frame_variant(r, false).small);
    r = s;
    r.nee = NeeParams{kSome, 1, 0};
    CHECK(!frame_variant(r, false).small);
    CHECK(!frame_variant(scene(0), false).small);

    // the run-time compiled kind of each variant; none for BVH, statistics and no shape
    CHECK(same(jit_kind(PathsVariant{false, false, 1, 0, false, 0}, shape), JitKind{kJitPaths, 1}));
    CHECK(same(jit_kind(PathsVariant{false, false, 0, 0, true, 0}, shape), JitKind{kJitPathsChan, 0}));
    CHECK(same(jit_kind(PathsVariant{false, false, 2, 0, false, kNeeAll}, shape), JitKind{kJitPathsNee, 2}));
    CHECK(same(jit_kind(PathsVariant{false, true, 0, kBvhSmallWaves, false, 0}, shape), kJitNone));
    CHECK(same(jit_kind(PathsVariant{true, false, 0, 0, false, 0}, shape), kJitNone));
    CHECK(same(jit_kind(PathsVariant{false, false, 0, 0, false, 0}, 0), kJitNone));
    CHECK(same(jit_kind(FrameVariant{false, false, 0, false, 0, false}, shape), JitKind{kJitFrame, 0}));
    CHECK(same(jit_kind(FrameVariant{false, false, 2, false, kNeeAll, false}, shape), JitKind{kJitFrameNee, 2}));
    CHECK(same(jit_kind(FrameVariant{false, false, 1, false, 0, true}, shape), JitKind{kJitFrameRgba, 1}));
    CHECK(same(jit_kind(FrameVariant{false, false, 2, false, kNeeAll, true}, shape), JitKind{kJitFrameNeeRgba, 2}));
    CHECK(same(jit_kind(FrameVariant{false, true, 0, true, 0, false}, shape), kJitNone));
    CHECK(same(jit_kind(FrameVariant{true, false, 0, false, 0, false}, shape), kJitNone));
    CHECK(same(jit_kind(FrameVariant{false, false, 0, false, 0, true}, 0), kJitNone));
    JitKindList l = jit_kinds_of_scene(true, 1);
    CHECK(l.n == 2 && same(l.k[0], JitKind{kJitPathsNee, 2}) && same(l.k[1], JitKind{kJitFrameNee, 2}));
    l = jit_kinds_of_scene(false, 1);
    CHECK(l.n == 3 && same(l.k[0], JitKind{kJitPaths, 1}) && same(l.k[1], JitKind{kJitFrame, 1}) && same(l.k[2], JitKind{kJitPathsChan, 1}));
}

static void frame_grids() {
    const uint32_t Ps[] = {1, 63, 64, 65, 129, 14400, 262144, 921600, 2073600, 8294400};
    const uint32_t cus[] = {1, 8, 256};
    const int occs[] = {1, 5, 6, 7, 10};
    for (uint32_t P : Ps)
        for (uint32_t cu : cus)
            for (int occ : occs)
                for (uint32_t mode = 0; mode <= 3; ++mode)
                    for (uint32_t live : {0u, P / 3u, P})
                        for (bool bvh : {false, true}) {
                            const FrameGrid g = frame_grid(P, live, mode, bvh, occ, cu);
                            const uint32_t per_block = kBlock * kFrameSkyPerLane;
                            CHECK(g.sky_blocks == (mode == 3 ? (P - live + per_block - 1) / per_block : 0));
                            CHECK(g.path_grid >= 1 && g.path_grid <= (uint32_t)occ * cu);
                            const uint32_t units = mode == 3 ? live : P;
                            const uint32_t runs = (units + frame_chunk(bvh) - 1) / frame_chunk(bvh);
                            const uint32_t needed = std::max(1u, (runs + kBlockWaves - 1) / kBlockWaves);
                            if (bvh) {  // full occupancy, within the global stacks' sizing
                                CHECK(g.path_grid <= kMaxResidentWaves / kBlockWaves * cu);
                                CHECK(g.path_grid == std::min(needed, (uint32_t)std::min(occ, 8) * cu));
                            } else {  // ~4 runs per wave, with lists ~2 counted over the whole image; whole blocks per CU
                                const uint32_t all_runs = (P + kFrameRun - 1) / kFrameRun;
                                const uint32_t want = all_runs / ((mode == 3 ? kFrameListsRpw : kFrameRunsPerWave) * kBlockWaves);
                                const uint32_t per_cu = std::max(1u, std::min((uint32_t)occ, (want + cu / 2) / cu));
                                CHECK(g.path_grid == std::min(needed, per_cu * cu));
                            }
                        }
    // 1080p Cornell on 256 CUs at 6 blocks per CU: 16200 runs / 16 = 1012 blocks wanted -> 4 per CU
    CHECK(frame_grid(2073600, 0, 0, false, 6, 256).path_grid == 4 * 256);
    CHECK(frame_grid(2073600, 2073600, 3, false, 6, 256).path_grid == 6 * 256);
}

static void jit_names() {
    const uint64_t shape = flat_shape_key(0x1234, 20);
    const std::string sh = std::to_string((unsigned long long)shape) + "ull";
    CHECK(jit_name_expr(kJitPaths, 1, shape) == "spt::k_paths<false, false, 1, " + sh + ">");
    CHECK(jit_name_expr(kJitFrame, 1, shape) == "spt::k_frame<false, false, 1, " + sh + ">");
    CHECK(jit_name_expr(kJitPathsChan, 1, shape) == "spt::k_paths<false, false, 1, " + sh + ", 0, true>");
    CHECK(jit_name_expr(kJitPathsNee, 1, shape) == "spt::k_paths<false, false, 2, " + sh + ", 0, false, 1>");
    CHECK(jit_name_expr(kJitFrameNee, 1, shape) == "spt::k_frame<false, false, 2, " + sh + ", false, 1>");
    CHECK(jit_name_expr(kJitFrameRgba, 1, shape) == "spt::k_frame<false, false, 1, " + sh + ", false, 0, true>");
    CHECK(jit_name_expr(kJitFrameNeeRgba, 1, shape) == "spt::k_frame<false, false, 2, " + sh + ", false, 1, true>");
    CHECK(jit_name_expr(kJitPaths, 0, 68719476756ull) == "spt::k_paths<false, false, 0, 68719476756ull>");
    static_assert(kNeeAll == 1, "the kNee argument the NEE kinds' names spell");
}

int main() {
    chunk_plan_invariants();
    chunk_plan_values();
    selectors();
    frame_grids();
    jit_names();
    std::printf(g_failed ? "FAIL (%d checks)\n" : "PASS\n", g_failed);
    return g_failed ? 1 : 0;
}
