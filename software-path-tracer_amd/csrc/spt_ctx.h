// spt_ctx.h — the context behind the C-ABI (include/spt.h spt_ctx): its record, the device memory it owns and
// what every entry point starts from. Private to the HIP units that define entry points on a context:
// spt_capi.hip (the context itself, the scene, render, resolve) and spt_capi_post.hip (post-processing).
#pragma once

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <string>
#include <vector>

#include "scene.h"
#include "spt.h"
#include "spt_ctx_state.h"
#include "spt_dev_mem.h"
#include "spt_kernels.h"

namespace spt {

struct EventPair {
    hipEvent_t a = nullptr, b = nullptr;
    int kind = 0;  // 0 extend, 1 shade, 2 other, 3 tail, 4 persistent
    uint32_t bounce = 0;
    uint32_t launches = 1;  // kind 4: the launches between a and b (> 1 for a SPT_PROFILE_SPAN pair)
    // kind 4, a split launch (ViewHalf): the second half's pair, on its stream; the launch's time is
    // (latest end - earliest start) of the two pairs
    hipEvent_t a2 = nullptr, b2 = nullptr;
};

// One half of a split view (spt_launch_plan.h make_view_split): the k_paths launches over it run on a
// stream of their own, with everything a launch writes besides its pixels' sums kept per half.
struct ViewHalf {
    hipStream_t stream = nullptr;  // non-blocking, created with the ctx
    hipEvent_t done = nullptr;     // behind the half's last launch of a call: the ctx stream waits on it (the join)
    uint32_t* work = nullptr;      // 2 sets of kWorkWords of its own, inside the ctx's `work` (k_paths zeroes work_next
    uint32_t work_parity = 0;      // in stream order: a set is never shared across streams)
};

// ---- device memory: every allocation has an owner (spt_dev_mem.h), in the record of what frees it ----
struct HipAlloc {
    static void* alloc(size_t bytes) {
        void* p = nullptr;
        if (hipMalloc(&p, bytes) == hipSuccess) return p;
        (void)hipGetLastError();  // (the caller reports the failure: no sticky error is left for a later check)
        return nullptr;
    }
    static void free(void* p) { (void)hipFree(p); }
};
template <class T>
using Dev = DevBuf<T, HipAlloc>;

// The scene's: freed by free_scene (spt_set_scene, a failed upload, spt_destroy).
struct SceneMem {
    Dev<float4> d_prims;
    Dev<float4> d_mats;
    Dev<float4> d_nodes;
    Dev<float4> d_emit;  // SPT_FLAG_NEE: the sampled emitters (scene.h DevEmitter), n_emit records
    Dev<uint32_t> d_mat_map;  // the caller's material index behind each device material (h_dev_mat)
    // one word per material of h_mats, 0 for a METAL or DIELECTRIC one; uploaded by spt_reproject while some
    // model is not DIFFUSE (bsdf)
    Dev<uint32_t> d_reusable;
    Dev<uint8_t> bvh_stack;  // the persistent kernels' traversal stacks (global memory)
};

// The configuration's, each sized by it: freed by free_buffers (a reallocating spt_configure, spt_destroy), so
// none outlives the size it was allocated for. What spt_configure does not allocate, the first call that
// writes it does.
struct ConfigMem {
    Dev<float4> q_o[2], q_d[2], q_t[2];
    Dev<float2> hit;
    Dev<float4> radiance;
    Dev<float4> accum;
    Dev<float2> hit_cache;  // k_frame: each shard pixel's camera-segment closest hit
    Dev<uint16_t> chunk_cost;  // flat k_paths' first-tier chunk costs and order (PassParams)
    Dev<uint32_t> chunk_order;
    struct {  // ... and each half's of a split view, [pixels / 2 + 64] (its key: DerivedState::half_order_key)
        Dev<uint16_t> cost;
        Dev<uint32_t> order;
    } half_mem[2];
    // Flat k_paths' view lists (spt_kernels.h ViewPlan): every pixel's bounce 0, compacted into live-pixel
    // records and constant pixels. Built behind the first persistent launch that finds them dropped; the
    // persistent launches that follow run over them. spt_reset keeps them: it only zeroes the sums.
    Dev<float4> view_live;      // [3 * pixels]
    Dev<float4> view_const;     // [pixels]
    Dev<uint32_t> view_counts;  // [2] live, constant; then the compaction's per-block scratch
    Dev<uint4> live_rec;        // hit_cache compacted: the live pixels' records (kFrameHitCache 2)
    Dev<uint32_t> sky_pix;      // ... the sky pixels' indices
    Dev<uint32_t> list_counts;  // [2] live, sky; then the compaction's per-block scratch
    Dev<uint32_t> resolved;
    // sorted ray queues (SPT_FLAG_SORTED_RAYS)
    Dev<uint16_t> ray_keys;
    Dev<uint32_t> ray_perm, ray_bins, ray_cursor;
    Dev<float4> feat_a, feat_b, feat_albedo;  // spt_render_features: the first-hit images
    Dev<float4> dn[2];                        // spt_denoise: the filter's two ping-pong images
    Dev<float> dn_var[2];                     // spt_denoise_guided: the variance planes that go with them
    // Temporal reprojection. spt_history_capture: the captured view — image with lengths, feat_a, feat_b in
    // 3 * pixels float4, laid out as hist_view_layout says (spt_reproject.h)
    Dev<float4> hist_view;
    Dev<float4> hist;         // spt_reproject: the active history (rgb, length)
    Dev<float4> blend;        // spt_history_blend: the blended image
    Dev<float4> noise_state;  // spt_noise_update: the per-pixel moments
    Dev<float> noise_e2;      // spt_noise_meter: the e2 image
};

// The context's own: freed by spt_destroy (gather_buf by free_comm as well).
struct OwnMem {
    Dev<uint32_t> counts;
    Dev<unsigned long long> totals;
    Dev<uint32_t> work;  // k_paths / k_frame work heads: 2 sets of kWorkWords, alternating per launch; then two per view half
    Dev<float4> d_env;   // octahedral environment map (spt_set_env_map) or empty
    Dev<float4> d_camera;  // the camera's device record (PassParams::cam_pose), allocated by the first spt_set_camera
    // The luminance meter and the display transform: scratch only, nothing a change could make stale. The 256
    // device words a metering sums into and the staging image of spt_resolve_display_device_image (grown on demand)
    Dev<uint32_t> meter_counts;
    Dev<uint32_t> display_stage;
    Dev<float4> gather_buf;  // rank 0: comm_ranks padded shards; other ranks: their padded shard
};

}  // namespace spt

struct spt_ctx : spt::SceneMem, spt::ConfigMem, spt::OwnMem {  // (as bases: a buffer is c->accum, whichever record holds it)
    int device = -1;
    hipStream_t own_stream = nullptr;
    // The stream the caller's work is ordered on. Everything but the split launches' join reaches it through
    // on_stream(), which marks it dirty for the next split launch's fork (stream_dirty below).
    hipStream_t user_stream = nullptr;
    // Split k_paths launches (spt_tuning.split_streams): a view's lists in two halves on two streams.
    spt::ViewHalf half[2];
    hipEvent_t fork_ev = nullptr;   // on the ctx stream: what the half streams wait on after anything else ran there
    // Set by every use of the ctx stream (on_stream) — every entry point that enqueues on it, drains it before
    // changing what a launch reads, or replaces it — and cleared by a split launch's fork: two split renders
    // with nothing between them fork without a wait, so call k+1's halves overlap call k's.
    bool stream_dirty = true;
    int32_t split_streams = 0;      // spt_tuning: -1 never, 0 automatic, 1 always when a view is valid
    bool last_view_split = false;   // the last persistent launch was split
    bool last_view_wide = false;    // ... ran the wide kernel (64-pixel chunks)
    int32_t wide_chunks = 0;        // spt_tuning: 0 = automatic, 1 = every eligible launch over a view, -1 = never
    // spt_accum_device_ptr handed the sums' address out (until the next spt_configure frees it): the caller may
    // read them with work of its own on its stream that no ctx call sees, so every split launch forks, as if
    // the stream were always dirty (it then waits for that work; the overlap across calls is given up)
    bool accum_shared = false;
    std::string err;
    uint32_t cu_count = 256;
    spt::DerivedState derived;  // which of the results cached below are valid (spt_ctx_state.h: what each change drops)

    // scene (its device arrays: SceneMem)
    uint32_t n_emit = 0;          // records in d_emit
    uint32_t n_emit_spheres = 0;  // ... of which spheres (NeeParams::spheres)
    uint32_t env_w = 0, env_h = 0;
    uint32_t n_prims = 0, n_nodes = 0, n_mats = 0;
    uint32_t n_dev_nodes = 0;  // records in d_nodes (4-wide, quantized): bounds the kernels' LDS top-node copies
    uint32_t bvh_stack_need = 0;  // the most stack entries a traversal of the 4-wide tree holds (bvh4_stack_need)
    uint32_t bvh_stack_stride = 0;  // entries per lane in bvh_stack (bvh_stack_stride(need)); 0: none allocated
    uint32_t bvh_stack_tb = 1;      // 4-B stack entries: bits of the entry-distance code (bvh_stack_t0_bits)
    spt_env env{};
    bool has_scene = false;
    uint32_t flat_ends = 0;  // PassParams::flat_ends
    uint32_t flat_rect = 0;  // flat_rect_bits of the kind-major copy (part of the shape key)
    uint32_t flat_pairs = 0; // flat_wall_pairs of the kind-major copy (part of the shape key)
    bool fast_div = false;  // scene.cpp fast_division_ok: the flat loop's unscaled divisions apply
    bool flat_ranges = false;  // scene.cpp flat_ranges_ok: the shape key's range bit (spt_kernels.h kShapeRanges)
    uint64_t scene_bytes = 0;
    uint64_t stack_bytes = 0;  // the persistent kernels' global traversal stacks (BVH scenes)

    // configuration
    spt_config cfg{};
    bool configured = false;
    uint32_t rows = 0;          // rows owned by this shard
    uint32_t pixels = 0;        // rows * width
    uint32_t frames_per_pass = 1;
    uint32_t n_sub = 0;         // block-private sub-queues (= blocks of every extend/shade launch)
    uint32_t sub_cap = 0;       // capacity of one sub-queue

    // what goes with the device buffers (ConfigMem, OwnMem)
    uint32_t view_n[2] = {0, 0};      // view_counts[0..1], read back once per build
    int32_t view_cache = 0;           // spt_tuning: 0 = automatic, -1 = never (every launch computes bounce 0 itself)
    bool last_view_cached = false;    // the last persistent launch ran over the lists
    uint32_t live_pixels = 0;         // list_counts[0], read back once per compaction
    uint32_t work_parity = 0;         // which of `work`'s two sets the next launch on the ctx stream takes
    uint32_t chunks_per_wave = 0;  // k_paths: chunks per resident wave in each small tail tier (spt_tuning; 0 = auto)
    uint32_t px_shift = 0;         // k_paths forced chunk size, log2 pixels (spt_tuning.px_shift = 2..5, clamped to the build)
    // spt_register_host_output: a caller's host image buffer, page-locked and mapped into the GPU's
    // address space, that the resolve kernel writes over PCIe directly (no device staging, no DMA copy)
    void* out_host = nullptr;
    void* out_dev = nullptr;
    size_t out_bytes = 0;
    // spt_render_resolve_rgba8: the resolve the next k_frame launch of spt_render fuses (fuse_frames != 0),
    // and whether a launch took it
    float fuse_frames = 0.0f, fuse_exposure = 1.0f;
    bool fused = false;

    uint32_t frame_count = 0;

    int dn_form = -1;  // spt_set_denoise_form: -1 the form measured faster at each step
    bool dn_guided = false;  // the denoised image is spt_denoise_guided's: dn_var[dn_result] is its variance
    // spt_history_capture: the captured view's (hist_view) layout and camera
    int hist_view_layout = 0;
    bool hist_view_has_camera = false;
    spt_camera hist_view_camera{};
    int hist_layout = -1;        // spt_set_history_layout: -1 the layout measured faster
    int meter_form = -1;         // spt_set_meter_form: -1 the form measured faster
    // The noise estimate (spt_noise_update / spt_noise_meter): the batches B and frames W folded into
    // noise_state since the accumulation last restarted (noise_frames: W as the caller counts it). spt_reset
    // clears the counts; an update that finds B = 0 zeroes the moments first.
    bool noise_metered = false;  // noise_e2 holds a metering of the current state's accumulation
    uint32_t noise_batches = 0, noise_frames = 0;
    float noise_W = 0.0f;

    // spt_set_camera: the posed camera, or none (the reference's pinhole at the origin); kept across spt_configure
    bool has_camera = false;
    spt_camera camera{};
    // spt_set_camera_lens: the camera's thin lens, or none; kept across spt_configure and spt_set_camera(cam)
    bool has_lens = false;
    spt_lens lens{};
    // BVH scenes: the reach of the ray origins the tree's boxes are padded for (scene.h; 0: the scene's own
    // magnitude) and that magnitude: spt_set_camera re-pads the tree when the camera leaves it or returns
    float pad_reach = 0.0f;
    float scene_mag = 1.0f;

    // spt_set_material_models: one model per material of h_mats, or empty (all DIFFUSE). The device
    // materials carry each model as one word (DevMaterial::albedo[3], spt_device.h model_kind); h_dm is
    // the uploaded array without them and h_dev_mat[i] the caller's material behind device material i
    // (a flat scene's materials are compacted). bsdf: some model is not DIFFUSE (PassParams::bsdf).
    std::vector<spt_material_model> h_models;
    std::vector<spt::DevMaterial> h_dm;
    std::vector<uint32_t> h_dev_mat;
    bool bsdf = false;

    // stats
    uint64_t frames = 0, paths = 0, passes = 0;
    bool profiling = false;
    bool span = false;        // SPT_PROFILE_SPAN: one event pair around the persistent launches
    bool span_open = false;   // its begin event is recorded
    spt::EventPair span_ev;
    std::vector<spt::EventPair> pending;
    std::vector<spt::EventPair> free_events;
    uint64_t ext_launches = 0, shade_launches = 0, ext_segments = 0;
    double ext_ms = 0.0, shade_ms = 0.0, other_ms = 0.0, tail_ms = 0.0;
    uint64_t tail_launches = 0;
    // Schedule (measured): flat scenes run one fused extend+shade launch per bounce
    // and finish paths from bounce 3 in k_trace_tail; BVH scenes run split extend/shade launches
    // for every bounce (traversal divergence makes the fused and tail kernels slower there).
    // Overrides: spt_tuning.fused / .tail_bounce (spt_set_tuning), or SPT_FLAG_SPLIT_KERNELS.
    int fused_override = -1;       // -1: automatic
    uint32_t tail_override = 0;    // 0: automatic
    double ext_ms_b[spt::kMaxBounces] = {}, shade_ms_b[spt::kMaxBounces] = {};
    // Calls of >= SPT_PERSISTENT_MIN_FRAMES frames run the persistent k_paths schedule instead
    // (SPT_FLAG_WAVEFRONT or spt_tuning.persistent = 0 keep the wavefront one).
    int persistent_override = -1;  // -1: automatic
    int frame_override = -1;       // spt_tuning.frame_kernel for calls of < SPT_PERSISTENT_MIN_FRAMES frames
    bool counters = false;         // SPT_PROFILE_COUNTERS: k_paths tallies segments per bounce
    double persist_ms = 0.0;
    uint64_t persist_launches = 0;
    uint32_t last_schedule = SPT_SCHEDULE_FUSED;
    uint32_t sub_alloc = 0;        // n_sub the queue buffers were sized for (spt_configure)
    uint32_t bvh_max_leaf = 0;     // spt_tuning: 0 = bvh_max_leaf(n)
    uint32_t bvh_bins = 0;         // spt_tuning: 0 = the builder's default
    int32_t specialize = 0;        // spt_tuning: flat scenes' kernels compiled for their shape: 0 = in the
                                   // background (generic kernels until ready), 1 = inside the first launch, -1 = never
    // sorted ray queues (SPT_FLAG_SORTED_RAYS): the binning grid over the BVH scene's bounds
    float scene_lo[3] = {0.f, 0.f, 0.f}, scene_hi[3] = {1.f, 1.f, 1.f};
    // host copies of the current scene for spt_update_prims: the caller's arrays, and for a BVH scene
    // the device-order records and the binary tree (refitted, not rebuilt, on an edit)
    std::vector<spt_prim> h_prims;
    std::vector<spt_material> h_mats;
    std::vector<spt::DevPrim> h_dp;
    std::vector<spt::BvhNode> h_nodes;
    std::vector<uint32_t> h_pos;  // original primitive index -> its record's position on the device
    bool last_specialized = false; // the last persistent / frame launch ran the specialized kernel
    uint32_t last_pairs = 0;       // ... whose key held this many wall pairs (flat_shape_pairs)
    bool last_ranges = false;      // ... a k_paths whose step loop ran its guard-free forms (flat_ranges_baked)

    // multi-GPU (spt_comm_init / spt_gather_image)
    ncclComm_t comm = nullptr;
    int comm_ranks = 0, comm_rank = -1;
    // spt_gather_image_overlapped: the gather runs on a stream of its own while the ctx stream renders on
    hipStream_t comm_stream = nullptr;
    hipEvent_t snap_ready = nullptr;   // ctx stream: the shard snapshot is in gather_buf
    hipEvent_t gather_done = nullptr;  // comm stream: the last overlapped gather (and assembly) finished
    bool gather_pending = false;       // an overlapped gather was enqueued since the last wait
};

namespace spt {

// The ctx stream, for anything that is about to enqueue on it, wait for it or replace it: the one place
// that marks it dirty (spt_ctx::stream_dirty). Only the split launches' join takes user_stream directly.
inline hipStream_t& on_stream(spt_ctx* c) {
    c->stream_dirty = true;
    return c->user_stream;
}

inline int fail(spt_ctx* c, int code, const std::string& msg) {
    if (c) c->err = msg;
    return code;
}

#define SPT_HIP(ctx, call)                                                                   \
    do {                                                                                     \
        hipError_t e_ = (call);                                                              \
        if (e_ != hipSuccess)                                                                \
            return fail((ctx), SPT_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_)); \
    } while (0)

// buf holds exactly n elements (kept if it does already), or SPT_ERR_HIP and "<who>: allocation failed"
template <class T>
int ensure_buf(spt_ctx* c, Dev<T>& buf, size_t n, const char* who) {
    if (buf.ensure(n)) return SPT_OK;
    return fail(c, SPT_ERR_HIP, std::string(who) + ": allocation failed");
}

inline hipError_t wait_frame(spt_ctx* c) { return hipStreamSynchronize(on_stream(c)); }
// The ctx's image as RGBA8 in host_out, waited for; launch(out, stream) enqueues the kernel that writes it.
template <class Launch>
int resolve_image_by(spt_ctx* c, uint32_t* host_out, Launch&& launch) {
    SPT_HIP(c, hipSetDevice(c->device));
    if (c->pixels == 0) return SPT_OK;
    if (host_out == c->out_host && sizeof(uint32_t) * (size_t)c->pixels <= c->out_bytes) {
        // the registered buffer: the kernel's stores go straight to host memory over PCIe
        launch((uint32_t*)c->out_dev, on_stream(c));
        SPT_HIP(c, hipGetLastError());
    } else {
        launch(c->resolved, on_stream(c));
        SPT_HIP(c, hipGetLastError());
        SPT_HIP(c, hipMemcpyAsync(host_out, c->resolved, sizeof(uint32_t) * c->pixels, hipMemcpyDeviceToHost, on_stream(c)));
    }
    SPT_HIP(c, wait_frame(c));
    return SPT_OK;
}

// img / divisor as RGBA8 in host_out, waited for (the sums and a frame count, or a mean and 1)
inline int resolve_image(spt_ctx* c, const float4* img, float divisor, float exposure, uint32_t* host_out) {
    return resolve_image_by(c, host_out, [&](uint32_t* out, hipStream_t s) {
        launch_resolve(img, c->pixels, divisor, exposure, out, s);
    });
}

PassParams base_params(spt_ctx* c);  // the launch parameters of the current scene and configuration (spt_capi.hip)

}  // namespace spt
