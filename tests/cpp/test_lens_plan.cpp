// the launch plan of a lens camera (spt_launch_plan.h): kCamLens on kCamPosed or kCamJitter plans exactly
// as kCamJitter does, and the cameras without a lens plan as they did
#include <cstdio>
#include "spt_launch_plan.h"
using namespace spt;
static int g_fail = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); ++g_fail; } } while (0)
static PassParams scene(uint32_t n_prims, bool bvh, uint32_t n_emit, uint32_t spheres, bool env, uint32_t cam_mode,
                        uint32_t bsdf) {
    static float4 dummy;
    PassParams p{};
    p.n_prims = n_prims;
    p.nodes = bvh ? &dummy : nullptr;
    p.nee = NeeParams{&dummy, n_emit, spheres};
    p.env = env ? &dummy : nullptr;
    p.cam_mode = cam_mode;
    p.bsdf = bsdf;
    p.rgba = nullptr;
    return p;
}
int main() {
    // the modes' values are part of the device record
    static_assert(kCamReference == 0u && kCamPosed == 1u && kCamJitter == 2u && kCamLens == 4u, "camera modes");
    CHECK(!cam_per_path(kCamReference) && !cam_per_path(kCamPosed) && cam_per_path(kCamJitter));
    CHECK(cam_per_path(kCamPosed | kCamLens) && cam_per_path(kCamJitter | kCamLens));
    const uint64_t shape = jit_config_key(flat_shape_key(0x2082082u, 8u), 8u, 2u, 1u, 0u, true);
    const uint32_t lens_modes[2] = {kCamPosed | kCamLens, kCamJitter | kCamLens};
    uint32_t rgba_word = 0;
    for (uint32_t bsdf = 0; bsdf < 2; ++bsdf)
        for (int stats = 0; stats < 2; ++stats)
            for (int bvh = 0; bvh < 2; ++bvh)
                for (int env = 0; env < 2; ++env)
                    for (uint32_t emit = 0; emit < 3; ++emit)
                        for (int rgba = 0; rgba < 2; ++rgba)
                            for (uint32_t shift = 0; shift <= kMaxChunkShift; ++shift) {
                                const uint32_t n = bvh ? 1000u : 8u, sph = emit == 2u ? 1u : 0u;
                                PassParams j = scene(n, bvh, emit, sph, env, kCamJitter, bsdf);
                                j.rgba = rgba ? &rgba_word : nullptr;
                                const PathsVariant vj = paths_variant(j, stats, shift);
                                const FrameVariant fj = frame_variant(j, stats);
                                for (const uint32_t mode : lens_modes) {
                                    PassParams l = j;
                                    l.cam_mode = mode;
                                    const PathsVariant v = paths_variant(l, stats, shift);
                                    const FrameVariant f = frame_variant(l, stats);
                                    CHECK(v == vj && f == fj);
                                    CHECK(v.bsdf == (bsdf != 0u) && f.bsdf == (bsdf != 0u));  // with bsdf: the bsdf form
                                    CHECK(bsdf ? !v.jitter : v.jitter);
                                    CHECK(f.jitter);
                                    CHECK(v.env == 2 && v.simd_waves == 0 && !v.chan);
                                    CHECK(jit_form(v, bvh ? 0ull : shape) == kNoJitForm);
                                    CHECK(jit_form(f, bvh ? 0ull : shape) == jit_form(fj, bvh ? 0ull : shape));
                                    for (int cv = 0; cv < 2; ++cv)
                                        for (int li = 0; li <= cv; ++li) {
                                            CHECK(frame_hit_mode(l, cv, li) == 0u);
                                            CHECK(frame_hit_mode(l, cv, li) == frame_hit_mode(j, cv, li));
                                        }
                                    CHECK(!view_lists_scene(l) && view_lists_scene(l) == view_lists_scene(j));
                                }
                                // kCamReference and kCamPosed: as they were (the jitter field off, the hit modes, the
                                // view lists of a flat scene without material models)
                                for (const uint32_t mode : {kCamReference, kCamPosed}) {
                                    PassParams q = j;
                                    q.cam_mode = mode;
                                    const PathsVariant v = paths_variant(q, stats, shift);
                                    const FrameVariant f = frame_variant(q, stats);
                                    CHECK(!v.jitter && !f.jitter && v.bsdf == (bsdf != 0u) && f.bsdf == (bsdf != 0u));
                                    if (!bsdf) {
                                        const bool nee = emit != 0u;
                                        CHECK(v.env == (nee ? 2 : env));
                                        CHECK(v.simd_waves == ((bvh && !stats && !nee) ? kBvhSmallWaves : 0));
                                        CHECK(v.chan == (!bvh && !stats && !nee && shift < kMaxChunkShift));
                                        CHECK(frame_hit_mode(q, false, false) == 1u && frame_hit_mode(q, true, false) == 2u &&
                                              frame_hit_mode(q, true, true) == 3u);
                                    } else {
                                        CHECK(frame_hit_mode(q, true, true) == 0u);
                                    }
                                    CHECK(view_lists_scene(q) == (!bvh && !bsdf));
                                }
                            }
    if (g_fail == 0) std::puts("ok");
    return g_fail ? 1 : 0;
}
