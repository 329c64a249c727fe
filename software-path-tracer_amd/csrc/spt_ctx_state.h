// spt_ctx_state.h — what a context (spt_capi.hip spt_ctx) caches between calls: which results are valid, and
// which results each change drops. The one statement of that rule in code (DESIGN.md "What a change drops"
// holds the same matrix); tests/cpp/test_ctx_state.cpp pins it without a GPU. Pure host code, no HIP. Internal.
#pragma once

#include <cstdint>

namespace spt {

enum Derived : uint32_t {     // the cached results, a bit each
    kCameraHits = 1u << 0,    // k_frame's camera-segment hit per pixel, and the lists compacted from them (kFrameLists)
    kChunkOrder = 1u << 1,    // k_paths' first-tier chunk costs and order: valid while chunk_order_key != 0
    kViewLists = 1u << 2,     // flat k_paths' view lists: every pixel's bounce 0
    kFeatures = 1u << 3,      // the first-hit feature images
    kDenoised = 1u << 4,      // the denoised image: valid while dn_result >= 0
    kCapturedView = 1u << 5,  // spt_history_capture's image, features and camera
    kHistory = 1u << 6,       // spt_reproject's active history
    kBlended = 1u << 7,       // spt_history_blend's image
    kReusable = 1u << 8,      // spt_reproject's uploaded word per material
    // ... and what goes with the buffers alone
    kHalfOrders = 1u << 9,     // the view halves' chunk orders (half_order_key)
    kViewNoMemory = 1u << 10,  // the view lists' allocation failed: the pixel plan runs, no second attempt
    kFrameLists = 1u << 11,    // k_frame takes the compacted lists (hit_mode 3): set and dropped with kCameraHits only
};

enum class Change {  // what changed: dropped by the entry point that changed it
    Scene,           // with the scene's memory (spt_capi.hip SceneMem): spt_set_scene, spt_destroy, a failed upload
    Prims,           // spt_update_prims (a flat scene goes on through spt_set_scene: Scene too)
    Configuration,   // spt_configure, always
    Buffers,         // with the configuration's memory (ConfigMem): a reallocating spt_configure, spt_destroy
    Sky,             // spt_set_env_map
    Camera,          // spt_set_camera
    Lens,            // spt_set_camera_lens
    Materials,       // spt_set_material_models
    Counters,        // spt_set_profiling, when SPT_PROFILE_COUNTERS changes
    HistoryClear,    // spt_history_clear
};

constexpr uint32_t kPrimary = kCameraHits | kChunkOrder | kViewLists;  // what k_frame and k_paths keep of bounce 0
constexpr uint32_t kHistories = kCapturedView | kHistory;
constexpr uint32_t kDrops[] = {  // by Change
    // other geometry: other camera hits, chunk costs, first hits and radiance; the per-material words go with the
    // materials. The denoised and blended images stay readable: they are images of what was rendered
    /* Scene */ kPrimary | kFeatures | kHistories | kReusable,
    /* Prims */ kPrimary | kFeatures | kHistories,
    // another size, shard, flags or bounce limit: nothing is of this configuration yet
    /* Configuration */ kPrimary | kFeatures | kDenoised | kHistories | kBlended,
    /* Buffers */ kPrimary | kFeatures | kDenoised | kHistories | kBlended | kHalfOrders | kViewNoMemory,
    // the view lists hold the sky pixels' radiance and the histories the old sky's light; the camera hits stay
    /* Sky */ kViewLists | kHistories,
    // another view: the active history was mapped into the previous one; spt_reproject maps the captured view
    /* Camera */ kPrimary | kFeatures | kHistory,
    // as Camera, but the feature images are the chief ray's, whatever the lens
    /* Lens */ kPrimary | kHistory,
    // other kernels (kBsdf: no cache, no lists) and other radiance; the first hits do not depend on the models
    /* Materials */ kPrimary | kHistories | kReusable,
    // the compacted lists were chosen for the kernels of the old counters setting
    /* Counters */ kCameraHits | kViewLists,
    /* HistoryClear */ kHistories,
};
static_assert(sizeof(kDrops) == sizeof(uint32_t) * ((unsigned)Change::HistoryClear + 1u), "a row per Change");

struct DerivedState {
    uint32_t bits = 0;
    uint64_t chunk_order_key = 0;         // the plan the whole view's order was sorted for (launch_paths writes it), 0: none
    uint64_t half_order_key[2] = {0, 0};  // ... each half's of a split view
    int dn_result = -1;                   // which of the two denoise images holds the result, -1: none

    bool valid(Derived item) const {
        return item == kChunkOrder ? chunk_order_key != 0 : item == kDenoised ? dn_result >= 0 : (bits & item) != 0;
    }
    bool frame_lists() const { return (bits & kFrameLists) != 0; }

    void drop(Change why) { clear(kDrops[(int)why]); }
    // a producer is about to overwrite `item`: invalid until produced (a failed launch leaves it so)
    void begin(Derived item) { clear(item); }
    void produced(Derived item) { bits |= item; }  // kFeatures, kCapturedView, kHistory, kBlended, kReusable, kViewNoMemory
    void produced_camera_hits(bool lists) { bits = (bits & ~(uint32_t)kFrameLists) | kCameraHits | (lists ? kFrameLists : 0u); }
    void produced_view_lists() {  // (the halves' chunk orders were the old lists'; the whole view's key stays)
        bits |= kViewLists;
        half_order_key[0] = half_order_key[1] = 0;
    }
    void produced_denoised(int image) { dn_result = image; }
    void clear(uint32_t m) {
        if (m & kCameraHits) m |= kFrameLists;
        bits &= ~m;
        if (m & kChunkOrder) chunk_order_key = 0;
        if (m & kHalfOrders) half_order_key[0] = half_order_key[1] = 0;
        if (m & kDenoised) dn_result = -1;
    }
};

}  // namespace spt
