// the launch plan of a camera (spt_launch_plan.h): which k_paths / k_frame forms a jittered pass picks
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
    return p;
}
int main() {
    const uint64_t shape = jit_config_key(flat_shape_key(0x2082082u, 8u), 8u, 2u, 1u, 0u);
    for (int stats = 0; stats < 2; ++stats)
        for (int bvh = 0; bvh < 2; ++bvh)
            for (int env = 0; env < 2; ++env)
                for (uint32_t emit = 0; emit < 3; ++emit)
                    for (uint32_t shift = 0; shift <= kMaxChunkShift; ++shift) {
                        // emit 1: emitters without a sphere; 2: with one
                        const PassParams j = scene(bvh ? 1000u : 8u, bvh, emit, emit == 2u ? 1u : 0u, env, kCamJitter);
                        const PathsVariant v = paths_variant(j, stats, shift);
                        CHECK(v.jitter);                              // the kJitter form ...
                        CHECK(v.env == 2 && v.simd_waves == 0 && !v.chan);  // ... generic: no 8-wave, no channel-lane kernel
                        CHECK(v.stats == (stats != 0) && v.bvh == (bvh != 0));
                        CHECK(v.nee == (emit == 0u ? 0 : (bvh && emit == 1u ? kNeeNoSpheres : kNeeAll)));
                        CHECK(jit_form(v, bvh ? 0ull : shape) == kNoJitForm);  // no shape-specialized kernel
                        const FrameVariant f = frame_variant(j, stats);
                        CHECK(f.jitter);
                        // the hit cache and the lists are ignored, whatever the ctx holds
                        CHECK(frame_hit_mode(j, false, false) == 0u && frame_hit_mode(j, true, false) == 0u &&
                              frame_hit_mode(j, true, true) == 0u);
                        // a posed camera plans exactly as the reference camera does
                        const PassParams r = scene(bvh ? 1000u : 8u, bvh, emit, emit == 2u ? 1u : 0u, env, kCamReference);
                        PassParams q = r;
                        q.cam_mode = kCamPosed;
                        const PathsVariant a = paths_variant(r, stats, shift), b = paths_variant(q, stats, shift);
                        CHECK(!a.jitter && !b.jitter && a == b);
                        CHECK(jit_form(a, bvh ? 0ull : shape) == jit_form(b, bvh ? 0ull : shape));
                        CHECK(!frame_variant(q, stats).jitter);
                        CHECK(frame_hit_mode(q, false, false) == 1u && frame_hit_mode(q, true, false) == 2u &&
                              frame_hit_mode(q, true, true) == 3u);
                    }
    // the small-BVH and channel-lane forms exist for the other cameras (so the checks above are not vacuous)
    CHECK(paths_variant(scene(1000u, true, 0u, 0u, false, kCamPosed), false, 5u).simd_waves == kBvhSmallWaves);
    CHECK(paths_variant(scene(8u, false, 0u, 0u, false, kCamPosed), false, 3u).chan);
    CHECK(jit_form(paths_variant(scene(8u, false, 0u, 0u, false, kCamPosed), false, 5u), shape) == jit_form_of(PathsVariant{false, false, 0, 0, false, 0}));
    if (g_fail == 0) std::puts("ok");
    return g_fail ? 1 : 0;
}
