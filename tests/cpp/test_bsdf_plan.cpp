// the launch plan of a scene with material models (spt_launch_plan.h): without models it is field for
// field the plan of before; with them every persistent launch takes its kBsdf form
#include <cstdio>
#include "spt_launch_plan.h"
using namespace spt;
static int g_fail = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); ++g_fail; } } while (0)
static PassParams scene(uint32_t n_prims, bool bvh, uint32_t n_emit, uint32_t spheres, bool env, uint32_t cam_mode) {
    static float4 dummy;
    PassParams p{};
    p.n_prims = n_prims;
    p.nodes = bvh ? &dummy : nullptr;
    p.nee = NeeParams{&dummy, n_emit, spheres};
    p.env = env ? &dummy : nullptr;
    p.cam_mode = cam_mode;
    p.cu_count = 256;
    p.shard_pixels = 1920u * 1080u;
    return p;
}
// the plan as it was before the models existed, restated: what paths_variant / frame_variant must still give
static PathsVariant paths_before(const PassParams& p, bool stats, uint32_t first_shift) {
    const bool bvh = p.nodes != nullptr;
    const int nee = p.nee.n_emit == 0u ? 0 : (bvh && p.nee.spheres == 0u ? kNeeNoSpheres : kNeeAll);
    PathsVariant v{stats, bvh, nee ? 2 : (p.env ? 1 : 0), 0, false, nee};
    if (p.cam_mode == kCamJitter) {
        v.env = 2;
        v.jitter = true;
        return v;
    }
    if (bvh && !stats && !nee && p.n_prims <= kBvhSmall) v.simd_waves = kBvhSmallWaves;
    v.chan = !bvh && !stats && !nee && first_shift < kMaxChunkShift;
    return v;
}
int main() {
    const uint64_t shape = jit_config_key(flat_shape_key(0x2082082u, 8u), 8u, 2u, 1u, 0u);
    for (int stats = 0; stats < 2; ++stats)
        for (int bvh = 0; bvh < 2; ++bvh)
            for (int env = 0; env < 2; ++env)
                for (uint32_t emit = 0; emit < 3; ++emit)
                    for (uint32_t cam = kCamReference; cam <= kCamJitter; ++cam)
                        for (uint32_t shift = 0; shift <= kMaxChunkShift; ++shift)
                            for (int rgba = 0; rgba < 2; ++rgba) {
                                static uint32_t out;
                                // emit 1: emitters without a sphere; 2: with one
                                PassParams r = scene(bvh ? 1000u : 8u, bvh, emit, emit == 2u ? 1u : 0u, env, cam);
                                r.rgba = rgba ? &out : nullptr;
                                // ---- without models: the plan of before, field for field
                                const PathsVariant a = paths_variant(r, stats, shift);
                                CHECK(a == paths_before(r, stats, shift) && !a.bsdf);
                                const JitForm ka = jit_form(a, bvh ? 0ull : shape);
                                const bool generic = bvh || stats || cam == kCamJitter;
                                CHECK((ka == kNoJitForm) == generic);
                                // the NEE, the channel-lane or the plain form, with the variant's sky kind
                                if (!generic) CHECK(ka == jit_form_of(PathsVariant{false, false, a.env, 0, !emit && a.chan, emit ? kNeeAll : 0}));
                                const FrameVariant f = frame_variant(r, stats);
                                const bool fstats = stats && !rgba;
                                const int nee = emit == 0u ? 0 : (bvh && emit == 1u ? kNeeNoSpheres : kNeeAll);
                                CHECK(!f.bsdf && f.stats == fstats && f.bvh == (bvh != 0) && f.env == (nee ? 2 : env) &&
                                      f.small == frame_small_scene(r, fstats) && f.nee == nee && f.rgba == (rgba != 0) &&
                                      f.jitter == (cam == kCamJitter));
                                const JitForm kf = jit_form(f, bvh ? 0ull : shape);
                                CHECK((kf == kNoJitForm) == (bvh || fstats));
                                if (kf) CHECK(kf == jit_form_of(FrameVariant{false, false, f.env, false, f.nee, f.rgba}));
                                if (cam != kCamJitter)
                                    CHECK(frame_hit_mode(r, false, false) == 1u && frame_hit_mode(r, true, false) == 2u &&
                                          frame_hit_mode(r, true, true) == 3u);
                                // ---- with models: the kBsdf forms
                                PassParams m = r;
                                m.bsdf = 1u;
                                const PathsVariant b = paths_variant(m, stats, shift);
                                CHECK(b.bsdf && !b.jitter && b.env == 2 && b.simd_waves == 0 && !b.chan);  // one generic form ...
                                CHECK(b.stats == (stats != 0) && b.bvh == (bvh != 0));
                                CHECK(b.nee == (emit ? kNeeAll : 0));  // ... that samples every emitter kind
                                CHECK(jit_form(b, bvh ? 0ull : shape) == kNoJitForm);  // no shape-specialized kernel
                                const FrameVariant g = frame_variant(m, stats);
                                CHECK(g.bsdf && g.env == 2 && !g.small && g.nee == (emit ? kNeeAll : 0) && g.stats == fstats &&
                                      g.bvh == (bvh != 0) && g.rgba == (rgba != 0));
                                CHECK(jit_form(g, bvh ? 0ull : shape) == kNoJitForm);
                                // hit_mode 0: every camera segment is traced, whatever the ctx holds
                                CHECK(frame_hit_mode(m, false, false) == 0u && frame_hit_mode(m, true, false) == 0u &&
                                      frame_hit_mode(m, true, true) == 0u);
                            }
    // a BVH scene small enough for k_frame's LDS-held form loses it with models
    PassParams s = scene(38u, true, 0u, 0u, false, kCamReference);
    s.n_dev_nodes = 13u;
    s.n_mats = 1u;
    s.stack_need = 6u;
    CHECK(frame_variant(s, false).small);
    s.bsdf = 1u;
    CHECK(!frame_variant(s, false).small && frame_variant(s, false).bsdf);
    if (g_fail == 0) std::puts("ok");
    return g_fail ? 1 : 0;
}
