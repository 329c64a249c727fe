// spt_launch_plan.h — what launch_paths / launch_frame decide before they launch: which instantiation
// of k_paths / k_frame runs, which the library holds, its run-time compiled form (spt_jit.h), the chunk plan and the grids.
// Pure host functions, no HIP runtime calls: tests/cpp/test_launch_plan.cpp checks them without a
// GPU. Every variant computes the same image bits, so a wrong choice here shows only as lost speed.
// Not part of the kernel source compiled at run time. Internal.
#pragma once

#include <algorithm>
#include <string>

#include "spt_jit.h"
#include "spt_kernels.h"

namespace spt {

// A form of the persistent kernels is described by one of these values and nothing else (shape: 0 in the
// library's own kernels, a flat scene's in the ones compiled at run time; k_frame's jitter is no argument):
// k_paths<stats, bvh, env, shape, simd_waves, chan, nee, jitter, bsdf, wide> / k_frame<stats, bvh, env, shape, small, nee, rgba, bsdf>
struct PathsVariant {
    bool stats, bvh;
    int env;         // 0 gradient sky, 1 environment map, 2 decided at run time (the NEE kernels)
    int simd_waves;  // 0, or kBvhSmallWaves: the 8-wave kernel of small BVH scenes
    bool chan;       // the channel-lane kernel of flat scenes whose chunks are all <= 16 pixels (a small row shard)
    int nee;         // 0, kNeeAll, or kNeeNoSpheres (a BVH scene without sphere lights)
    bool jitter = false;  // the kJitter form (a per-path camera ray: jittered, a lens, or both — cam_per_path): every path
                          // traces its camera segment; env 2 only
    bool bsdf = false;    // the kBsdf form (a scene with material models): starts every path at bounce 0 too and reads
                          // the camera's kind at run time, so `jitter` stays false; env 2, nee 0 or kNeeAll
    bool wide = false;    // the kWide form (64-pixel chunks over a view's lists): flat, pixel lanes, no NEE; env 0 or 1
};
struct FrameVariant {
    bool stats, bvh;
    int env;
    bool small;  // a BVH scene held whole in LDS (frame_small_scene)
    int nee;
    bool rgba;   // the resolve fused into the frame; it has no stats form
    bool jitter = false;  // a per-path camera ray (cam_per_path): the same kernels on hit_mode 0 (no camera-hit cache, no lists)
    bool bsdf = false;    // the kBsdf kernels (a scene with material models): hit_mode 0, env 2, never `small`
};
constexpr bool operator==(const PathsVariant& a, const PathsVariant& b) {
    return a.stats == b.stats && a.bvh == b.bvh && a.env == b.env && a.simd_waves == b.simd_waves && a.chan == b.chan &&
           a.nee == b.nee && a.jitter == b.jitter && a.bsdf == b.bsdf && a.wide == b.wide;
}
constexpr bool operator==(const FrameVariant& a, const FrameVariant& b) {
    return a.stats == b.stats && a.bvh == b.bvh && a.env == b.env && a.small == b.small && a.nee == b.nee &&
           a.rgba == b.rgba && a.jitter == b.jitter && a.bsdf == b.bsdf;
}

// A variant's code: its fields as the digits of a mixed-radix number, the first field the most significant
// (env and nee: 0, 1, 2; simd_waves: 0 or kBvhSmallWaves). paths_of_code / frame_of_code are the inverses:
// each field is the code over the product of the radices behind it, modulo its own.
constexpr int kPathsCodes = 2 * 2 * 3 * 2 * 2 * 3 * 2 * 2 * 2;
constexpr int kFrameCodes = 2 * 2 * 3 * 2 * 3 * 2 * 2 * 2;
constexpr int paths_code(const PathsVariant& v) {
    return (((((((v.stats * 2 + v.bvh) * 3 + v.env) * 2 + (v.simd_waves != 0)) * 2 + v.chan) * 3 + v.nee) * 2 + v.jitter) * 2 + v.bsdf) * 2 + v.wide;
}
constexpr PathsVariant paths_of_code(int c) {
    return PathsVariant{c / 576 % 2 != 0, c / 288 % 2 != 0, c / 96 % 3, c / 48 % 2 ? kBvhSmallWaves : 0, c / 24 % 2 != 0, c / 8 % 3,
                        c / 4 % 2 != 0, c / 2 % 2 != 0, c % 2 != 0};
}
constexpr int frame_code(const FrameVariant& v) {
    return ((((((v.stats * 2 + v.bvh) * 3 + v.env) * 2 + v.small) * 3 + v.nee) * 2 + v.rgba) * 2 + v.jitter) * 2 + v.bsdf;
}
constexpr FrameVariant frame_of_code(int c) {
    return FrameVariant{c / 288 % 2 != 0, c / 144 % 2 != 0, c / 48 % 3, c / 24 % 2 != 0, c / 8 % 3, c / 4 % 2 != 0, c / 2 % 2 != 0, c % 2 != 0};
}

// Whether the library holds a k_paths / k_frame of the variant (compiled offline, shape 0): the rules by which
// spt_kernels.hip instantiates its kernel table. paths_variant / frame_variant ask for these only.
constexpr bool paths_built(const PathsVariant& v) {
    if (v.bsdf || v.jitter || v.nee) {
        // the sky's kind read at run time (env 2); pixel lanes at the kernel's own occupancy, 32-pixel chunks at most
        if (v.env != 2 || v.simd_waves || v.chan || v.wide) return false;
        // kBsdf reads the camera's kind at run time (no kJitter of its own) and samples every emitter kind
        if (v.bsdf) return !v.jitter && v.nee != kNeeNoSpheres;
        return v.bvh || v.nee != kNeeNoSpheres;  // (the sphere sample is left out of BVH kernels only)
    }
    if (v.env == 2) return false;
    if (v.wide) return !v.bvh && !v.simd_waves && !v.chan;       // flat scenes over a view's lists, pixel lanes
    if (v.simd_waves) return v.bvh && !v.stats && !v.chan;       // small BVH scenes: 8 waves per SIMD
    if (v.chan) return !v.bvh && !v.stats;                       // flat scenes, chunks of <= 16 pixels
    return true;
}
// (`jitter` selects no kernel of its own: both values name the same instantiation)
constexpr bool frame_built(const FrameVariant& v) {
    if (v.rgba && v.stats) return false;  // the fused resolve has no stats form
    if (v.bsdf) return v.env == 2 && !v.small && v.nee != kNeeNoSpheres;
    if (v.nee) return v.env == 2 && !v.small && (v.bvh || v.nee == kNeeAll);
    if (v.env == 2) return false;
    return !v.small || (v.bvh && !v.stats);
}
// how many kernels that makes: 40 k_paths and 37 k_frame (a k_frame per built code without `jitter`)
constexpr int paths_built_count() {
    int n = 0;
    for (int c = 0; c < kPathsCodes; ++c) n += paths_built(paths_of_code(c));
    return n;
}
constexpr int frame_built_count() {
    int n = 0;
    for (int c = 0; c < kFrameCodes; ++c) n += !frame_of_code(c).jitter && frame_built(frame_of_code(c));
    return n;
}

inline int nee_variant(const PassParams& p) {
    if (p.nee.n_emit == 0u) return 0;
    return p.nodes != nullptr && p.nee.spheres == 0u ? kNeeNoSpheres : kNeeAll;
}
// first_shift: the chunk plan's shift[0]; wide: the launch runs a view's wide plan (wide_launch: flat, no NEE,
// a per-pixel camera ray, no material models)
inline PathsVariant paths_variant(const PassParams& p, bool stats, uint32_t first_shift, bool wide = false) {
    const bool bvh = p.nodes != nullptr;
    const int nee = nee_variant(p);
    PathsVariant v{stats, bvh, nee ? 2 : (p.env ? 1 : 0), 0, false, nee};
    if (p.bsdf) {  // one generic form per (stats, bvh, nee on or off), whatever the camera
        v.env = 2;
        v.nee = nee ? kNeeAll : 0;
        v.bsdf = true;
        return v;
    }
    if (cam_per_path(p.cam_mode)) {  // one generic form per (stats, bvh, nee): no 8-wave, no channel-lane kernel
        v.env = 2;
        v.jitter = true;
        return v;
    }
    if (bvh && !stats && !nee && p.n_prims <= kBvhSmall) v.simd_waves = kBvhSmallWaves;
    v.chan = !bvh && !stats && !nee && first_shift < kMaxChunkShift;
    v.wide = wide && !bvh && !nee;
    if (v.wide) v.chan = false;  // (its small tiers run in the wide kernel's pixel lanes)
    return v;
}
inline FrameVariant frame_variant(const PassParams& p, bool stats) {
    const bool rgba = p.rgba != nullptr;
    stats = stats && !rgba;
    const int nee = nee_variant(p);
    if (p.bsdf) return FrameVariant{stats, p.nodes != nullptr, 2, false, nee ? kNeeAll : 0, rgba, cam_per_path(p.cam_mode), true};
    return FrameVariant{stats, p.nodes != nullptr, nee ? 2 : (p.env ? 1 : 0), frame_small_scene(p, stats), nee, rgba,
                        cam_per_path(p.cam_mode)};
}
// k_frame's hit_mode for a launch: a jittered or lens camera's segment differs per frame, so its launches neither
// store nor read the camera-hit cache and take no lists, whatever the ctx holds; nor do the launches of a
// scene with material models (the kBsdf kernels trace every camera segment)
inline uint32_t frame_hit_mode(const PassParams& p, bool cache_valid, bool lists) {
    if (cam_per_path(p.cam_mode) || p.bsdf) return 0u;
    return !cache_valid ? 1u : (lists ? 3u : 2u);
}

// The variant's kernel compiled for a flat scene's shape (spt_jit.h): the flat variant it instantiates, with the
// fields that select nothing in it cleared, so that launches which run the same kernel ask for the same one.
// kNoJitForm: there is none (a BVH scene, a per-path camera ray, material models, or no shape), the
// offline-compiled kernel runs. k_frame's counting form has none. The counting k_paths of a shape with wall
// pairs (flat_shape_pairs) is compiled for the shape, on first use: it then runs the paired wall test the timed
// kernel runs, and counts its second passes.
constexpr JitForm kNoJitForm{false, -1};
constexpr JitForm jit_form_of(const PathsVariant& v) { return JitForm{false, paths_code(v)}; }
constexpr JitForm jit_form_of(const FrameVariant& v) { return JitForm{true, frame_code(v)}; }
inline JitForm jit_form(const PathsVariant& v, uint64_t shape) {
    if (!shape || v.bvh || v.jitter || v.bsdf || (v.stats && !flat_shape_pairs(shape))) return kNoJitForm;
    const bool nee = v.nee && !v.wide;  // (a flat scene's NEE kernel samples every emitter kind; its sky kind is read at run time)
    return jit_form_of(PathsVariant{v.stats, false, nee ? 2 : v.env, 0, v.chan && !v.stats && !v.wide && !nee, nee ? kNeeAll : 0, false, false, v.wide});
}
inline JitForm jit_form(const FrameVariant& v, uint64_t shape) {
    if (!shape || v.bvh || v.stats || v.bsdf) return kNoJitForm;
    return jit_form_of(FrameVariant{false, false, v.nee ? 2 : v.env, false, v.nee ? kNeeAll : 0, v.rgba});
}
// the name expression hiprtc instantiates for (form, shape): every template argument, from the variant
inline std::string jit_name_expr(JitForm form, uint64_t shape) {
    const auto b = [](bool x) { return std::string(x ? "true" : "false"); };
    const auto i = [](int x) { return std::to_string(x); };
    const auto name = [](const char* kernel, std::initializer_list<std::string> args) {
        std::string s;
        for (const std::string& a : args) s += (s.empty() ? std::string("spt::") + kernel + "<" : ", ") + a;
        return s + ">";
    };
    const std::string sh = std::to_string((unsigned long long)shape) + "ull";
    if (form.frame) {
        const FrameVariant v = frame_of_code(form.code);
        return name("k_frame", {b(v.stats), b(v.bvh), i(v.env), sh, b(v.small), i(v.nee), b(v.rgba), b(v.bsdf)});
    }
    const PathsVariant v = paths_of_code(form.code);
    return name("k_paths", {b(v.stats), b(v.bvh), i(v.env), sh, i(v.simd_waves), b(v.chan), i(v.nee), b(v.jitter), b(v.bsdf), b(v.wide)});
}
// The forms a flat scene's renders may ask for: compiled ahead by spt_set_scene, waited for by
// spt_specialize_scene. (The two kRgba forms are not in the list: a fused resolve compiles its kernel
// on first use. Adding them here is the whole change, but it changes what a scene change compiles.)
// wide: the ctx may run wide launches (wide_possible), so the wide k_paths is compiled ahead too
struct JitFormList {
    int n;
    JitForm f[4];
};
inline JitFormList jit_kinds_of_scene(bool nee, int env, bool wide = false) {
    if (nee) return {2, {jit_form_of(PathsVariant{false, false, 2, 0, false, kNeeAll}), jit_form_of(FrameVariant{false, false, 2, false, kNeeAll, false})}};
    const PathsVariant paths{false, false, env, 0, false, 0}, chan{false, false, env, 0, true, 0};
    JitFormList l{3, {jit_form_of(paths), jit_form_of(FrameVariant{false, false, env, false, 0, false}), jit_form_of(chan)}};
    if (wide) l.f[l.n++] = jit_form_of(PathsVariant{false, false, env, 0, false, 0, false, false, true});
    return l;
}

// k_paths chunk plan (order and cost unset): the largest chunks (32/16/8 ... pixels) that still give
// every resident wave >= 8, then ~chunks_per_wave chunks per wave of each smaller size at the end (a
// wave's last chunk is the launch's tail). A small row shard of a multi-GPU run gets small chunks,
// which it needs to fill the GPU at all. px_shift (spt_tuning) forces one size.
inline ChunkPlan make_chunk_plan(uint32_t P, uint32_t resident_waves, uint32_t chunks_per_wave, uint32_t px_shift) {
    ChunkPlan plan{};
    uint32_t s0 = kMaxChunkShift;
    while (s0 > kMinChunkShift && ((uint64_t)P >> s0) < 8ull * resident_waves) --s0;
    if (px_shift) s0 = std::max(kMinChunkShift, std::min(px_shift, kMaxChunkShift));
    const uint32_t s1 = s0 > kMinChunkShift ? s0 - 1u : kMinChunkShift, s2 = s1 > kMinChunkShift ? s1 - 1u : kMinChunkShift;
    plan.shift[0] = s0;
    plan.shift[1] = s1;
    plan.shift[2] = s2;
    if (px_shift || s0 == kMinChunkShift) {
        plan.n[0] = (uint32_t)(((uint64_t)P + (1u << s0) - 1u) >> s0);
        return plan;
    }
    const uint64_t tail = (uint64_t)chunks_per_wave * resident_waves;  // chunks per small tier
    const uint32_t c_px = (uint32_t)std::min<uint64_t>(P, tail << s2);
    const uint32_t b_px = (uint32_t)std::min<uint64_t>(P - c_px, tail << s1) & ~((1u << s1) - 1u);
    const uint32_t a_px = (P - c_px - b_px) & ~((1u << s0) - 1u);
    plan.n[0] = a_px >> s0;
    plan.n[1] = b_px >> s1;
    plan.start[1] = a_px;
    plan.start[2] = a_px + b_px;
    plan.n[2] = (P - a_px - b_px + (1u << s2) - 1u) >> s2;
    return plan;
}
// names the plan a recorded first-tier order belongs to (first-tier chunks, pixels, chunk size)
inline uint64_t chunk_order_key(const ChunkPlan& plan, uint32_t P) {
    return ((uint64_t)plan.n[0] << 37) | ((uint64_t)P << 5) | plan.shift[0];
}


// k_paths over a view's compacted lists (ViewPlan; flat scenes): the tiers laid over the `live` records
// of the live list, and ceil(constant / kViewSweep) sweep units for the constant list, queued behind the
// first tier (where the pixel plan hands out its zero-cost chunks).
// The first tier's chunk size is the pixel plan's, from shard_pixels: the rule counts chunks per resident
// wave of the whole image, and computed from the live count it falls to 8 pixels on Cornell 1080p
// (805,896 live of 2,073,600), which measured -19 %. Each small tier gets the pixel plan's chunks per
// wave scaled by the live fraction, so a wave's last chunks stay as many as they were per traced pixel
// (the pixel plan's tail tiers cover the image's last pixels whatever they hold: on Cornell 1080p its
// 8-pixel tier holds no live pixel at all).
// (measurement builds: -DSPT_VIEW_TIER8=0 leaves the smallest tier to the remainder, the one A/B of the
// view plan's tiers, profiles/view_cache_rates.txt; -DSPT_VIEW_TIER16=0 leaves the middle tier out as well, for
// the A/B under split launches, profiles/split_streams_rates.txt)
#ifndef SPT_VIEW_TIER8
#define SPT_VIEW_TIER8 1
#endif
#ifndef SPT_VIEW_TIER16
#define SPT_VIEW_TIER16 1
#endif
constexpr bool kViewTier8 = SPT_VIEW_TIER8 != 0;
constexpr bool kViewTier16 = SPT_VIEW_TIER16 != 0;
struct ViewChunkPlan {
    ChunkPlan plan;
    uint32_t n_sweep;
};
// wide (the kWide kernel; never with px_shift): a first tier of kWidePx-pixel chunks whatever the pixel plan's
// is, over tiers of 32 and 16 pixels sized by the same rule; the tiers below the first stay <= 32 pixels.
inline ViewChunkPlan make_view_plan(uint32_t shard_pixels, uint32_t live, uint32_t constant, uint32_t resident_waves,
                                    uint32_t chunks_per_wave, uint32_t px_shift, bool wide = false) {
    ViewChunkPlan vp{};
    ChunkPlan& plan = vp.plan;
    vp.n_sweep = (constant + kViewSweep - 1u) / kViewSweep;
    const ChunkPlan pixel_plan = make_chunk_plan(shard_pixels, resident_waves, chunks_per_wave, px_shift);
    wide = wide && !px_shift;
    const uint32_t s0 = wide ? kWideShift : pixel_plan.shift[0], s1 = wide ? kWideShift - 1u : pixel_plan.shift[1],
                   s2 = wide ? kWideShift - 2u : pixel_plan.shift[2];
    plan.shift[0] = s0;
    plan.shift[1] = s1;
    plan.shift[2] = s2;
    if (px_shift || s0 == kMinChunkShift) {
        plan.n[0] = (uint32_t)(((uint64_t)live + (1u << s0) - 1u) >> s0);
        return vp;
    }
    // chunks per small tier
    const uint64_t tail = shard_pixels ? (uint64_t)chunks_per_wave * resident_waves * live / shard_pixels : 0u;
    // (a wide plan's small tiers take a quarter of the live list each at most, so its first tier exists: the cap
    // binds only where wide chunks are forced on an image below the automatic rule's — there the pixel plan's
    // first tier is 32 pixels, P >= 256 x the resident waves, so tail << s1 <= chunks_per_wave x live / 8)
    const uint64_t cap = wide ? live / 4u : live;
    const uint32_t c_px = kViewTier8 ? (uint32_t)std::min<uint64_t>(cap, tail << s2) : 0u;
    const uint32_t b_px = kViewTier16 ? (uint32_t)std::min<uint64_t>(std::min<uint64_t>(cap, live - c_px), tail << s1) & ~((1u << s1) - 1u) : 0u;
    const uint32_t a_px = (live - c_px - b_px) & ~((1u << s0) - 1u);
    plan.n[0] = a_px >> s0;
    plan.n[1] = b_px >> s1;
    plan.start[1] = a_px;
    plan.start[2] = a_px + b_px;
    plan.n[2] = (live - a_px - b_px + (1u << s2) - 1u) >> s2;
    return vp;
}
// names the view plan a recorded first-tier order belongs to (never a pixel plan's key: the top bit);
// half: 0 the whole view's plan, 1 / 2 the plan of half A / B of a split view (make_view_split): bits 61-62,
// which chunk_order_key leaves free for any first tier of < 2^24 chunks
inline uint64_t view_order_key(const ChunkPlan& plan, uint32_t live, uint32_t half = 0u) {
    return (chunk_order_key(plan, live) & ~(3ull << 61)) | ((uint64_t)(half & 3u) << 61) | (1ull << 63);
}

// A view's lists cut into two halves, A and B, that two k_paths launches on two streams run over at the
// same time (spt_capi.hip): the launches touch disjoint pixels, so nothing orders one against the other,
// and each launch's blocks move in as the other's waves run out of chunks. Half h covers live records
// [live_at[h], live_at[h + 1]) and constant pixels [const_at[h], const_at[h + 1]). The live list is cut at
// the multiple of the first tier's chunk size (first_tier_px, the whole shard's: make_view_plan) nearest
// its middle, the constant list at the multiple of kViewSweep nearest its middle, so no chunk and no
// sweep unit straddles the cut. A list shorter than half a unit goes to B whole: a half may be empty (and
// is then not launched).
struct ViewSplit {
    uint32_t live_at[3];
    uint32_t const_at[3];
};
inline uint32_t split_cut(uint32_t n, uint32_t unit) {
    unit = std::max(unit, 1u);
    const uint64_t cut = ((uint64_t)n / 2u + unit / 2u) / unit * unit;
    return (uint32_t)std::min<uint64_t>(cut, n);
}
// (first_tier_px: 1 << kMaxChunkShift, or kWidePx for a call whose launches may be wide — a multiple of every
// smaller chunk size, so the cut suits a launch of the call that runs the narrow plan after all)
inline ViewSplit make_view_split(uint32_t n_live, uint32_t n_const, uint32_t first_tier_px = 1u << kMaxChunkShift) {
    return ViewSplit{{0u, split_cut(n_live, first_tier_px), n_live}, {0u, split_cut(n_const, kViewSweep), n_const}};
}
// Whether the launches of one spt_render call over a cached view are split (spt_tuning.split_streams: knob).
// Decided ONCE per call, from the call's largest launch (a call of more than max_launch_frames frames runs
// several launches, the last one the remainder): were it decided per launch, a short remainder would run
// whole on the ctx stream while the halves of the launch before it are still in flight over the same pixels.
// Automatic (knob 0): launches of at least 2^24 live-pixel frames. The second launch and its ordering cost a
// call 13-18 us whatever its size, the overlap gains about 5 % of its time: measured +4.6 %
// at Cornell 1080p x 64 frames (51.6 M), +3.4 % on its 1/8 row shard x 512 frames (51.6 M), +6.5 % at 720p x
// 64 (22.9 M); -4.5 % at 480x270 x 64 (3.2 M), -25 % at 96x64 x 64 (0.15 M).
constexpr uint64_t kSplitMinLiveFrames = 1ull << 24;
inline bool split_call_wanted(int32_t knob, uint32_t n_live, uint32_t call_frames, uint32_t max_launch_frames) {
    if (knob) return knob > 0;
    return (uint64_t)n_live * std::min(call_frames, max_launch_frames) >= kSplitMinLiveFrames;
}
// Wide launches (spt_tuning.wide_chunks: knob; the kWide k_paths, 64-pixel chunks over a view's lists).
// Eligible: a flat scene with a per-pixel camera ray and no material models (the view's lists exist), no NEE,
// no forced chunk size, and a whole image: a row shard's launches hold world x the frames over 1 / world of the
// pixels and need their small chunks (make_chunk_plan), so they keep them (not measured otherwise).
// wide_call: decided once per call, as the split is (the cut of the live list and the frames per launch follow
// it): 0 no, 1 automatic (each launch then checks that the pixel plan's first tier is 32 pixels with the
// occupancy it asked: wide_launch), 2 forced on. Automatic: an image whose pixel plan starts with 32-pixel
// chunks (wide_first_tier: with the flat kernels' 7 blocks per CU) and launches of at least kWideMinLiveFrames
// live-pixel frames. Forced on against forced off at Cornell 1080p: 4 frames per call (3.2 M, the
// persistent schedule's shortest call) +21.8 %, 8 (6.4 M) +14.5 %, 16 (12.9 M) +5.7 %, 32 (25.8 M) +5.3 %, 64 (51.6 M) +1.9 to +2.6 %, 128 (103 M) +0.4 %; 4K x 16 (51.6 M)
// +13.7 %; 720p x 64, whose plan starts with 16-pixel chunks, -15 %. The threshold sits just below the smallest
// launch measured; nothing was measured below it.
constexpr uint64_t kWideMinLiveFrames = 3ull << 20;  // 3.15 M
constexpr int kWideBlocksPerCu = 7;  // the flat k_paths' blocks per CU (7 waves/SIMD), for the per-call estimate
inline bool wide_first_tier(uint32_t shard_pixels, uint32_t cu_count) {
    return make_chunk_plan(shard_pixels, (uint32_t)kWideBlocksPerCu * cu_count * (kBlock / 64u), 0u, 0u).shift[0] == kMaxChunkShift;
}
// The halves of a split view run without small tiers (spt_capi.hip launch_paths_split). A wide half has half as
// many first-tier chunks — Cornell 1080p: 6,296 for 7,168 resident waves — so its end is coarser, and one
// chunk per wave and small tier (32 and 16 pixels) pays: C2 +0.6 % over none, 2 chunks the same as none
// (profiles/wide_chunks_rates.txt).
constexpr uint32_t kWideSplitChunksPerWave = 1;
inline bool wide_eligible(const PassParams& p) {
    return view_lists_scene(p) && nee_variant(p) == 0 && p.shard_count <= 1u && p.px_shift == 0u;
}
inline int wide_call(int32_t knob, bool eligible, bool first_tier_32, uint32_t n_live, uint32_t call_frames) {
    if (knob < 0 || !eligible) return 0;
    if (knob > 0) return 2;
    return first_tier_32 && (uint64_t)n_live * std::min(call_frames, kWideMaxFrames) >= kWideMinLiveFrames ? 1 : 0;
}
inline bool wide_launch(int wide_call, uint32_t pixel_first_shift) {
    return wide_call == 2 || (wide_call == 1 && pixel_first_shift == kMaxChunkShift);
}
// whether a ctx of this many shard pixels can run a wide launch at all (its kernel is then compiled ahead)
inline bool wide_possible(int32_t knob, uint32_t shard_pixels, uint32_t shard_count, uint32_t cu_count) {
    if (knob < 0 || shard_count > 1u) return false;
    return knob > 0 || (wide_first_tier(shard_pixels, cu_count) && (uint64_t)shard_pixels * kWideMaxFrames >= kWideMinLiveFrames);
}
inline bool view_half_empty(const ViewSplit& s, uint32_t h) {
    return s.live_at[h + 1] == s.live_at[h] && s.const_at[h + 1] == s.const_at[h];
}

constexpr uint32_t kBlockWaves = kBlock / 64u;
// waves resident at once, from the occupancy query's blocks per CU
inline uint32_t resident_waves(int per_cu, uint32_t cu_count) { return (uint32_t)per_cu * cu_count * kBlockWaves; }
// k_paths: a persistent grid, as many blocks as are resident at once (the waves then pull chunks), but
// no more waves than chunks (a BVH scene's global traversal stacks are sized for kMaxResidentWaves per CU);
// sweep_units: a view plan's sweep units count as chunks
inline uint32_t paths_grid(const ChunkPlan& plan, bool bvh, int per_cu, uint32_t cu_count, uint32_t sweep_units = 0u) {
    const uint32_t chunks = plan.n[0] + plan.n[1] + plan.n[2] + sweep_units;
    const uint32_t needed = (chunks + kBlockWaves - 1u) / kBlockWaves;
    if (bvh) per_cu = std::min<int>(per_cu, (int)(kMaxResidentWaves / kBlockWaves));
    return std::min<uint32_t>(needed, (uint32_t)per_cu * cu_count);
}

// k_frame: a persistent grid, but no more waves than runs of frame_chunk() pixels (hit_mode 3: the live
// pixels are the work units; the sky pixels go to blocks of their own, kFrameSkyPerLane pixels per lane,
// launched ahead of the tracing blocks: blockIdx < sky_blocks).
// Flat scenes: a one-frame launch is bound by its lanes' longest chains of path segments, not by
// throughput (VALU issue ~0.34), so fewer resident waves, each taking ~kFrameRunsPerWave
// runs, finish the frame sooner than full occupancy (Cornell one frame per call: 720p 90 -> 67 us,
// 1080p 113 -> 98 us, 4K 238 -> 234 us). BVH scenes keep full occupancy (their latency-bound
// traversal needs the waves: C4 -4 % with the rule).
constexpr uint32_t kFrameRunsPerWave = 4;
constexpr uint32_t kFrameListsRpw = 2;  // flat scenes with lists: runs per wave, counted over the whole image's runs
struct FrameGrid {
    uint32_t path_grid, sky_blocks;
};
inline FrameGrid frame_grid(uint32_t shard_pixels, uint32_t live_pixels, uint32_t hit_mode, bool bvh, int per_cu,
                            uint32_t cu_count) {
    const bool lists = hit_mode == 3u;
    const uint32_t units = lists ? live_pixels : shard_pixels;
    const uint32_t runs = (units + frame_chunk(bvh) - 1u) / frame_chunk(bvh);
    if (!bvh) {
        // with lists (hit_mode 3) the rule counts the whole image's runs, so a wave takes about
        // kFrameListsRpw x the live fraction runs of live pixels
        const uint32_t rule_runs = lists ? (shard_pixels + frame_chunk(bvh) - 1u) / frame_chunk(bvh) : runs;
        const uint32_t rpw = lists ? kFrameListsRpw : kFrameRunsPerWave;
        const uint32_t want_blocks = rule_runs / (rpw * kBlockWaves);
        per_cu = std::max(1, std::min(per_cu, (int)((want_blocks + cu_count / 2u) / std::max(1u, cu_count))));
    }
    const uint32_t needed = (runs + kBlockWaves - 1u) / kBlockWaves;
    if (bvh) per_cu = std::min<int>(per_cu, (int)(kMaxResidentWaves / kBlockWaves));  // global stacks' sizing
    const uint32_t n_sky = lists ? shard_pixels - live_pixels : 0u;
    return FrameGrid{std::max(1u, std::min<uint32_t>(needed, (uint32_t)per_cu * cu_count)),
                     (n_sky + kBlock * kFrameSkyPerLane - 1u) / (kBlock * kFrameSkyPerLane)};
}

}  // namespace spt
