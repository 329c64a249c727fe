// Host check of the persistent kernels' launch planning (spt_launch_plan.h): the chunk plan of k_paths,
// which instantiation of k_paths / k_frame a scene runs, that the library holds it, its run-time compiled
// form and that form's name expression (jit_name_expr), and k_frame's grid. Every variant computes the same
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
// (operator== compares every field: jitter, bsdf and wide too)
template <class V>
static bool same(const V& a, const V& b) {
    return a == b;
}
// the run-time compiled form of `v` is the variant `want`
static bool jit_is(const PathsVariant& v, uint64_t shape, const PathsVariant& want) {
    const JitForm f = jit_form(v, shape);
    return f && !f.frame && paths_of_code(f.code) == want;
}
static bool jit_is(const FrameVariant& v, uint64_t shape, const FrameVariant& want) {
    const JitForm f = jit_form(v, shape);
    return f && f.frame && frame_of_code(f.code) == want;
}

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

    // the run-time compiled form of each variant; none for BVH, statistics (a shape without wall pairs) and no shape
    const uint64_t pairs = flat_shape_key(0, 20, 0, 1);  // (a shape with a wall pair: its counting k_paths is compiled too)
    CHECK(flat_shape_pairs(pairs) != 0 && flat_shape_pairs(shape) == 0);
    const PathsVariant plain{false, false, 1, 0, false, 0}, chan{false, false, 0, 0, true, 0}, nee{false, false, 2, 0, false, kNeeAll};
    const PathsVariant wide{false, false, 1, 0, false, 0, false, false, true}, wide_stats{true, false, 0, 0, false, 0, false, false, true};
    const PathsVariant stats{true, false, 0, 0, false, 0}, nee_stats{true, false, 2, 0, false, kNeeAll};
    CHECK(jit_is(plain, shape, plain));
    CHECK(jit_is(chan, shape, chan));
    CHECK(jit_is(nee, shape, nee));
    CHECK(jit_is(wide, shape, wide));
    CHECK(jit_is(stats, pairs, stats));
    CHECK(jit_is(nee_stats, pairs, nee_stats));
    CHECK(jit_is(wide_stats, pairs, wide_stats));
    CHECK(jit_form(PathsVariant{false, true, 0, kBvhSmallWaves, false, 0}, shape) == kNoJitForm);
    CHECK(jit_form(stats, shape) == kNoJitForm);
    CHECK(jit_form(nee_stats, shape) == kNoJitForm);
    CHECK(jit_form(wide_stats, shape) == kNoJitForm);
    CHECK(jit_form(PathsVariant{false, false, 0, 0, false, 0}, 0) == kNoJitForm);
    CHECK(jit_form(PathsVariant{false, false, 2, 0, false, 0, true}, shape) == kNoJitForm);         // jitter
    CHECK(jit_form(PathsVariant{false, false, 2, 0, false, 0, false, true}, shape) == kNoJitForm);  // bsdf
    const FrameVariant frame{false, false, 0, false, 0, false}, frame_nee{false, false, 2, false, kNeeAll, false};
    const FrameVariant frame_rgba{false, false, 1, false, 0, true}, frame_nee_rgba{false, false, 2, false, kNeeAll, true};
    CHECK(jit_is(frame, shape, frame));
    CHECK(jit_is(frame_nee, shape, frame_nee));
    CHECK(jit_is(frame_rgba, shape, frame_rgba));
    CHECK(jit_is(frame_nee_rgba, shape, frame_nee_rgba));
    CHECK(jit_is(FrameVariant{false, false, 0, false, 0, false, true}, shape, frame));  // jitter: the same kernel
    CHECK(jit_form(FrameVariant{false, true, 0, true, 0, false}, shape) == kNoJitForm);
    CHECK(jit_form(FrameVariant{true, false, 0, false, 0, false}, shape) == kNoJitForm);
    CHECK(jit_form(FrameVariant{true, false, 0, false, 0, false}, pairs) == kNoJitForm);  // k_frame's counting form: never
    CHECK(jit_form(FrameVariant{false, false, 0, false, 0, true}, 0) == kNoJitForm);
    CHECK(jit_form(FrameVariant{false, false, 2, false, 0, false, false, true}, shape) == kNoJitForm);  // bsdf
    JitFormList l = jit_kinds_of_scene(true, 1);
    CHECK(l.n == 2 && l.f[0] == jit_form_of(nee) && l.f[1] == jit_form_of(frame_nee));
    l = jit_kinds_of_scene(false, 1);
    CHECK(l.n == 3 && l.f[0] == jit_form_of(plain) && l.f[1] == jit_form_of(FrameVariant{false, false, 1, false, 0, false}) &&
          l.f[2] == jit_form_of(PathsVariant{false, false, 1, 0, true, 0}));
    l = jit_kinds_of_scene(false, 0, true);
    CHECK(l.n == 4 && l.f[0] == jit_form_of(PathsVariant{false, false, 0, 0, false, 0}) && l.f[1] == jit_form_of(frame) &&
          l.f[2] == jit_form_of(chan) && l.f[3] == jit_form_of(PathsVariant{false, false, 0, 0, false, 0, false, false, true}));
    l = jit_kinds_of_scene(true, 0, true);
    CHECK(l.n == 2 && l.f[0] == jit_form_of(nee) && l.f[1] == jit_form_of(frame_nee));
}

// The code of a variant and the forms the library holds: the pack / unpack pair over the whole code space, the
// counts, and every PassParams combination the selectors distinguish — each gets a built form, and its
// run-time compiled form, when there is one, is a built flat form.
static void forms_exhaustive() {
    static_assert(paths_built_count() == 40 && frame_built_count() == 37, "the forms the library holds");
    int n_paths = 0, n_frame = 0;
    for (int c = 0; c < kPathsCodes; ++c) {
        const PathsVariant v = paths_of_code(c);
        CHECK(paths_code(v) == c && same(paths_of_code(paths_code(v)), v));
        CHECK(v.env >= 0 && v.env <= 2 && v.nee >= 0 && v.nee <= 2 && (v.simd_waves == 0 || v.simd_waves == kBvhSmallWaves));
        n_paths += paths_built(v);
        if (v.wide && (v.bsdf || v.jitter || v.nee)) CHECK(!paths_built(v));
    }
    for (int c = 0; c < kFrameCodes; ++c) {
        const FrameVariant v = frame_of_code(c);
        CHECK(frame_code(v) == c && same(frame_of_code(frame_code(v)), v));
        CHECK(v.env >= 0 && v.env <= 2 && v.nee >= 0 && v.nee <= 2);
        FrameVariant j = v;
        j.jitter = !v.jitter;
        CHECK(frame_built(j) == frame_built(v));  // jitter selects no kernel of its own
        n_frame += !v.jitter && frame_built(v);
    }
    CHECK(n_paths == 40 && n_frame == 37);
    CHECK(paths_code(PathsVariant{true, true, 2, kBvhSmallWaves, true, 2, true, true, true}) == kPathsCodes - 1);
    CHECK(frame_code(FrameVariant{true, true, 2, true, 2, true, true, true}) == kFrameCodes - 1);

    const uint64_t shapes[] = {flat_shape_key(0, 20), flat_shape_key(0, 20, 0, 1)};  // without and with a wall pair
    static float4 pose[4];
    int combos = 0;
    for (int sc = 0; sc < 4; ++sc)  // flat / small BVH / large BVH / a BVH scene k_frame holds in LDS
        for (bool env : {false, true})
            for (int em = 0; em < 3; ++em)  // emitters: none / with spheres / without spheres
                for (uint32_t cam : {kCamReference, kCamPosed, kCamJitter, kCamPosed | kCamLens, kCamJitter | kCamLens})
                    for (bool bsdf : {false, true})
                        for (bool stats : {false, true})
                            for (bool rgba : {false, true})
                                for (uint32_t shift : {5u, 4u, 0u})
                                    for (bool wide : {false, true})
                                        for (uint64_t shape : shapes) {
                                            PassParams p = scene(sc == 0 ? 0 : sc == 1 ? kBvhSmall : sc == 2 ? 1000 : kFrameTopPrims,
                                                                 em ? 3 : 0, em == 1 ? 1 : 0, env);
                                            if (sc == 3) {
                                                p.n_dev_nodes = kFrameTopNodes;
                                                p.n_mats = 0;
                                                p.stack_need = kFrameLdsStackMax;
                                            }
                                            if (sc != 0) shape = 0;
                                            p.jit_shape = shape;
                                            p.cam_mode = cam;
                                            p.cam_pose = cam == kCamReference ? nullptr : pose;
                                            p.bsdf = bsdf ? 1u : 0u;
                                            p.rgba = rgba ? g_rgba : nullptr;
                                            ++combos;
                                            const PathsVariant v = paths_variant(p, stats, shift, wide);
                                            CHECK(paths_built(v));
                                            CHECK(v.stats == stats && v.bvh == (sc != 0));
                                            const JitForm jp = jit_form(v, shape);
                                            if (jp) {
                                                const PathsVariant f = paths_of_code(jp.code);
                                                CHECK(!jp.frame && !f.bvh && paths_built(f) && f.stats == v.stats && f.wide == v.wide);
                                            }
                                            const FrameVariant fv = frame_variant(p, stats);
                                            CHECK(frame_built(fv));
                                            CHECK(fv.bvh == (sc != 0) && fv.rgba == rgba);
                                            if (sc == 3 && !em && !bsdf && !(stats && !rgba)) CHECK(fv.small);
                                            const JitForm jf = jit_form(fv, shape);
                                            if (jf) {
                                                const FrameVariant f = frame_of_code(jf.code);
                                                CHECK(jf.frame && !f.bvh && !f.stats && !f.jitter && frame_built(f) && f.rgba == fv.rgba);
                                            }
                                        }
    CHECK(combos == 4 * 2 * 3 * 5 * 2 * 2 * 2 * 3 * 2 * 2);
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
    // (every template argument is spelled, the defaulted ones too: the same specializations as without them)
    const auto paths_name = [&](const PathsVariant& v, uint64_t s = 0) { return jit_name_expr(jit_form(v, s ? s : shape), s ? s : shape); };
    const auto frame_name = [&](const FrameVariant& v) { return jit_name_expr(jit_form(v, shape), shape); };
    CHECK(paths_name(PathsVariant{false, false, 1, 0, false, 0}) == "spt::k_paths<false, false, 1, " + sh + ", 0, false, 0, false, false, false>");
    CHECK(frame_name(FrameVariant{false, false, 1, false, 0, false}) == "spt::k_frame<false, false, 1, " + sh + ", false, 0, false, false>");
    CHECK(paths_name(PathsVariant{false, false, 1, 0, true, 0}) == "spt::k_paths<false, false, 1, " + sh + ", 0, true, 0, false, false, false>");
    CHECK(paths_name(PathsVariant{false, false, 2, 0, false, kNeeAll}) == "spt::k_paths<false, false, 2, " + sh + ", 0, false, 1, false, false, false>");
    CHECK(frame_name(FrameVariant{false, false, 2, false, kNeeAll, false}) == "spt::k_frame<false, false, 2, " + sh + ", false, 1, false, false>");
    CHECK(frame_name(FrameVariant{false, false, 1, false, 0, true}) == "spt::k_frame<false, false, 1, " + sh + ", false, 0, true, false>");
    CHECK(frame_name(FrameVariant{false, false, 2, false, kNeeAll, true}) == "spt::k_frame<false, false, 2, " + sh + ", false, 1, true, false>");
    CHECK(paths_name(PathsVariant{false, false, 0, 0, false, 0}, 68719476756ull) ==
          "spt::k_paths<false, false, 0, 68719476756ull, 0, false, 0, false, false, false>");
    // wide; and the counting forms of a shape with a wall pair: plain, NEE, wide
    CHECK(paths_name(PathsVariant{false, false, 1, 0, false, 0, false, false, true}) == "spt::k_paths<false, false, 1, " + sh + ", 0, false, 0, false, false, true>");
    const uint64_t pairs = flat_shape_key(0x1234, 20, 0, 1);
    const std::string ps = std::to_string((unsigned long long)pairs) + "ull";
    CHECK(paths_name(PathsVariant{true, false, 1, 0, false, 0}, pairs) == "spt::k_paths<true, false, 1, " + ps + ", 0, false, 0, false, false, false>");
    CHECK(paths_name(PathsVariant{true, false, 2, 0, false, kNeeAll}, pairs) == "spt::k_paths<true, false, 2, " + ps + ", 0, false, 1, false, false, false>");
    CHECK(paths_name(PathsVariant{true, false, 0, 0, false, 0, false, false, true}, pairs) == "spt::k_paths<true, false, 0, " + ps + ", 0, false, 0, false, false, true>");
    // a name spells whatever the code holds (the offline-only fields too)
    CHECK(jit_name_expr(jit_form_of(PathsVariant{false, true, 0, kBvhSmallWaves, false, kNeeNoSpheres, true, true, false}), 5ull) ==
          "spt::k_paths<false, true, 0, 5ull, " + std::to_string(kBvhSmallWaves) + ", false, 2, true, true, false>");
    CHECK(jit_name_expr(jit_form_of(FrameVariant{true, true, 0, true, 0, false}), 5ull) == "spt::k_frame<true, true, 0, 5ull, true, 0, false, false>");
    static_assert(kNeeAll == 1 && kNeeNoSpheres == 2, "the kNee argument the NEE forms' names spell");
}

int main() {
    chunk_plan_invariants();
    chunk_plan_values();
    selectors();
    frame_grids();
    jit_names();
    forms_exhaustive();
    std::printf(g_failed ? "FAIL (%d checks)\n" : "PASS\n", g_failed);
    return g_failed ? 1 : 0;
}
