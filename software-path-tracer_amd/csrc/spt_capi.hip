// spt_capi.hip — the C-ABI of libspt_hip.so (declared in include/spt.h).
//
// Owns one HIP device's state for the integrator: scene records, ray queues, accumulation, and
// the pass driver that replaces CPUPathTracer::render()'s serial pixel loop
// (libs/render/src/engines/pathtracer/backends/cpu/CPUPathTracer.cpp:43-85) with wavefront
// launches. Never aborts: every failure is a negative spt_status + spt_last_error().
#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "scene.h"
#include "spt.h"
#include "spt_ctx_state.h"
#include "spt_denoise.h"
#include "spt_denoise_guided.h"
#include "spt_dev_mem.h"
#include "spt_device.h"
#include "spt_display.h"
#include "spt_jit.h"
#include "spt_kernels.h"
#include "spt_launch_plan.h"
#include "spt_noise.h"
#include "spt_reproject.h"

using namespace spt;

static_assert(kBvhStackMax == kBvhStackEntries, "scene.h and spt_kernels.h stack bounds");
static_assert(kMatDiffuse == SPT_MAT_DIFFUSE && kMatMetal == SPT_MAT_METAL && kMatDielectric == SPT_MAT_DIELECTRIC,
              "spt.h spt_material_kind and spt_device.h model_kind");
static_assert(sizeof(spt_material_model) == 16, "spt_material_model is 16 bytes");
static_assert(sizeof(spt_denoise_params) == 32, "spt_denoise_params is 32 bytes");
static_assert(sizeof(spt_guided_params) == 32, "spt_guided_params is 32 bytes");
static_assert(sizeof(spt_reproject_params) == 32, "spt_reproject_params is 32 bytes");
static_assert(sizeof(spt_exposure_params) == 32, "spt_exposure_params is 32 bytes");
static_assert(sizeof(spt_display) == 16, "spt_display is 16 bytes");
static_assert(sizeof(spt_noise_params) == 16, "spt_noise_params is 16 bytes");

namespace {

// The tree the device traverses for a binary SAH BVH: its 4-wide collapse, quantized (scene.h BvhNodeQ),
// the most traversal stack entries it needs and the 4-B stack entries' t0 bits (bvh_stack_t0_bits of its
// largest child ref).
struct DevTree {
    std::vector<uint8_t> bytes;
    uint32_t stack_need = 0, stack_tb = 0;
};
template <int W, class Q, class QuantFn>
DevTree make_dev_tree(const std::vector<BvhNode>& bin, QuantFn quantize) {
    static_assert(sizeof(Q) == kDevNodeBytes, "device node record size");
    DevTree t;
    std::vector<BvhNodeW<W>> wide;
    collapse_bvh_w<W>(bin, wide);
    if (wide.empty()) return t;
    t.stack_need = bvh_w_stack_need<W>(wide, 0u);
    t.stack_tb = bvh_stack_t0_bits(bvh_w_max_ref<W>(wide));  // refs < 2^31 here
    std::vector<Q> q;
    quantize(wide, q);
    t.bytes.resize(sizeof(Q) * q.size());
    std::memcpy(t.bytes.data(), q.data(), t.bytes.size());
    return t;
}
DevTree device_tree(const std::vector<BvhNode>& bin) { return make_dev_tree<4, BvhNodeQ>(bin, quantize_bvh4); }

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

// float4s in n records of a device array the kernels address as float4 (scene.h DevPrim, DevMaterial, DevEmitter)
template <class Rec>
size_t float4s(size_t n) {
    static_assert(sizeof(Rec) % sizeof(float4) == 0, "a device record is whole float4s");
    return n * (sizeof(Rec) / sizeof(float4));
}
static_assert(kDevNodeBytes % sizeof(float4) == 0, "a device node is whole float4s");

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

}  // namespace

struct spt_ctx : SceneMem, ConfigMem, OwnMem {  // (as bases: a buffer is c->accum, whichever record holds it)
    int device = -1;
    hipStream_t own_stream = nullptr;
    // The stream the caller's work is ordered on. Everything but the split launches' join reaches it through
    // on_stream(), which marks it dirty for the next split launch's fork (stream_dirty below).
    hipStream_t user_stream = nullptr;
    // Split k_paths launches (spt_tuning.split_streams): a view's lists in two halves on two streams.
    ViewHalf half[2];
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
    DerivedState derived;  // which of the results cached below are valid (spt_ctx_state.h: what each change drops)

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
    std::vector<DevMaterial> h_dm;
    std::vector<uint32_t> h_dev_mat;
    bool bsdf = false;

    // stats
    uint64_t frames = 0, paths = 0, passes = 0;
    bool profiling = false;
    bool span = false;        // SPT_PROFILE_SPAN: one event pair around the persistent launches
    bool span_open = false;   // its begin event is recorded
    EventPair span_ev;
    std::vector<EventPair> pending;
    std::vector<EventPair> free_events;
    uint64_t ext_launches = 0, shade_launches = 0, ext_segments = 0;
    double ext_ms = 0.0, shade_ms = 0.0, other_ms = 0.0, tail_ms = 0.0;
    uint64_t tail_launches = 0;
    // Schedule (measured): flat scenes run one fused extend+shade launch per bounce
    // and finish paths from bounce 3 in k_trace_tail; BVH scenes run split extend/shade launches
    // for every bounce (traversal divergence makes the fused and tail kernels slower there).
    // Overrides: spt_tuning.fused / .tail_bounce (spt_set_tuning), or SPT_FLAG_SPLIT_KERNELS.
    int fused_override = -1;       // -1: automatic
    uint32_t tail_override = 0;    // 0: automatic
    double ext_ms_b[kMaxBounces] = {}, shade_ms_b[kMaxBounces] = {};
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
    std::vector<DevPrim> h_dp;
    std::vector<BvhNode> h_nodes;
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

namespace {

// The ctx stream, for anything that is about to enqueue on it, wait for it or replace it: the one place
// that marks it dirty (spt_ctx::stream_dirty). Only the split launches' join takes user_stream directly.
hipStream_t& on_stream(spt_ctx* c) {
    c->stream_dirty = true;
    return c->user_stream;
}

int fail(spt_ctx* c, int code, const std::string& msg) {
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

void free_buffers(spt_ctx* c) {
    static_cast<ConfigMem&>(*c) = {};
    c->noise_metered = false;
    c->derived.drop(Change::Buffers);
}

// RCCL, resolved at run time (spt.h): the copy already in the process (PyTorch loads its own
// librccl.so, soname librccl.so.1) or the ROCm install's. Linking one at build time could put two
// RCCLs in one process, whose exported symbols would interpose on each other.
struct Rccl {
    ncclResult_t (*get_unique_id)(ncclUniqueId*) = nullptr;
    ncclResult_t (*comm_init_rank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*gather)(const void*, void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*comm_destroy)(ncclComm_t) = nullptr;
    const char* (*error_string)(ncclResult_t) = nullptr;
    bool ok = false;
    std::string err;
};

const Rccl& rccl() {
    static const Rccl r = [] {
        Rccl x;
        void* h = nullptr;
        for (const char* name : {"librccl.so.1", "librccl.so"})
            if (!h) h = dlopen(name, RTLD_NOW | RTLD_NOLOAD);
        if (!h) h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
        if (!h) h = dlopen("/opt/rocm/lib/librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
        if (!h) {
            const char* e = dlerror();
            x.err = std::string("RCCL not found: ") + (e ? e : "dlopen failed");
            return x;
        }
        x.get_unique_id = (decltype(x.get_unique_id))dlsym(h, "ncclGetUniqueId");
        x.comm_init_rank = (decltype(x.comm_init_rank))dlsym(h, "ncclCommInitRank");
        x.gather = (decltype(x.gather))dlsym(h, "ncclGather");
        x.comm_destroy = (decltype(x.comm_destroy))dlsym(h, "ncclCommDestroy");
        x.error_string = (decltype(x.error_string))dlsym(h, "ncclGetErrorString");
        x.ok = x.get_unique_id && x.comm_init_rank && x.gather && x.comm_destroy && x.error_string;
        if (!x.ok) x.err = "RCCL: ncclGather / ncclCommInitRank missing from the loaded library";
        return x;
    }();
    return r;
}

#define SPT_NCCL(ctx, call)                                                                          \
    do {                                                                                             \
        ncclResult_t r_ = (call);                                                                    \
        if (r_ != ncclSuccess)                                                                       \
            return fail((ctx), SPT_ERR_HIP, std::string(#call) + ": " + rccl().error_string(r_));      \
    } while (0)

void free_comm(spt_ctx* c) {
    if (c->comm_stream) (void)hipStreamSynchronize(c->comm_stream);
    if (c->comm && rccl().ok) (void)rccl().comm_destroy(c->comm);
    if (c->snap_ready) (void)hipEventDestroy(c->snap_ready);
    if (c->gather_done) (void)hipEventDestroy(c->gather_done);
    if (c->comm_stream) (void)hipStreamDestroy(c->comm_stream);
    c->snap_ready = c->gather_done = nullptr;
    c->comm_stream = nullptr;
    c->gather_pending = false;
    c->comm = nullptr;
    c->comm_ranks = 0;
    c->comm_rank = -1;
    c->gather_buf.reset();
}

void free_scene(spt_ctx* c) {
    c->derived.drop(Change::Scene);
    static_cast<SceneMem&>(*c) = {};
    c->bvh_stack_stride = 0;
    c->n_prims = c->n_nodes = c->n_dev_nodes = c->n_emit = c->n_emit_spheres = 0;
    c->has_scene = false;
}

int flush_events(spt_ctx* c) {
    if (c->pending.empty()) return SPT_OK;
    SPT_HIP(c, hipEventSynchronize(c->pending.back().b));
    if (c->pending.back().b2) SPT_HIP(c, hipEventSynchronize(c->pending.back().b2));
    for (auto& e : c->pending) {
        float ms = 0.0f;
        if (e.a2) {
            // a split launch: from the earlier of the halves' starts to the later of their ends
            // (hipEventElapsedTime works between events of different streams)
            float lead = 0.0f, end_a = 0.0f, end_b = 0.0f;
            SPT_HIP(c, hipEventElapsedTime(&lead, e.a, e.a2));
            const hipEvent_t start = lead >= 0.0f ? e.a : e.a2;
            SPT_HIP(c, hipEventElapsedTime(&end_a, start, e.b));
            SPT_HIP(c, hipEventElapsedTime(&end_b, start, e.b2));
            ms = std::max(end_a, end_b);
        } else {
            SPT_HIP(c, hipEventElapsedTime(&ms, e.a, e.b));
        }
        if (e.kind == 0) {
            c->ext_ms += ms;
            c->ext_ms_b[e.bounce] += ms;
            c->ext_launches++;
        } else if (e.kind == 1) {
            c->shade_ms += ms;
            c->shade_ms_b[e.bounce] += ms;
            c->shade_launches++;
        } else if (e.kind == 3) {
            c->tail_ms += ms;
            c->tail_launches++;
        } else if (e.kind == 4) {
            c->persist_ms += ms;
            c->persist_launches += e.launches;
        } else {
            c->other_ms += ms;
        }
        if (e.a2) {  // back to the pool as the two pairs they were
            EventPair second;
            second.a = e.a2;
            second.b = e.b2;
            c->free_events.push_back(second);
            e.a2 = e.b2 = nullptr;
        }
        c->free_events.push_back(e);
    }
    c->pending.clear();
    return SPT_OK;
}

// a pair from the pool, nothing recorded yet
int take_events(spt_ctx* c, EventPair& out, int kind, uint32_t bounce = 0) {
    if (c->free_events.empty()) {
        EventPair e;
        SPT_HIP(c, hipEventCreate(&e.a));
        SPT_HIP(c, hipEventCreate(&e.b));
        c->free_events.push_back(e);
    }
    out = c->free_events.back();
    c->free_events.pop_back();
    out.kind = kind;
    out.bounce = bounce;
    out.launches = 1;  // (a pooled pair may have been a span)
    return SPT_OK;
}

int begin_event(spt_ctx* c, EventPair& out, int kind, uint32_t bounce = 0) {
    if (take_events(c, out, kind, bounce) != SPT_OK) return SPT_ERR_HIP;
    SPT_HIP(c, hipEventRecord(out.a, on_stream(c)));
    return SPT_OK;
}

int end_event(spt_ctx* c, EventPair& e) {
    SPT_HIP(c, hipEventRecord(e.b, on_stream(c)));
    c->pending.push_back(e);
    if (c->pending.size() >= 4096) return flush_events(c);
    return SPT_OK;
}

// A persistent (k_paths / k_frame) launch under profiling: its own event pair, or (SPT_PROFILE_SPAN)
// the span's begin before the first one and a launch counted
int begin_persistent(spt_ctx* c, EventPair& ev) {
    if (!c->profiling) return SPT_OK;
    if (!c->span) return begin_event(c, ev, 4);
    if (!c->span_open) {
        if (begin_event(c, c->span_ev, 4) != SPT_OK) return SPT_ERR_HIP;
        c->span_ev.launches = 0;
        c->span_open = true;
    }
    c->span_ev.launches++;
    return SPT_OK;
}

int end_persistent(spt_ctx* c, EventPair& ev) {
    if (!c->profiling || c->span) return SPT_OK;
    return end_event(c, ev);
}

// the span's end: after the last launch, recorded when the span mode is switched off
int close_span(spt_ctx* c) {
    if (!c->span_open) return SPT_OK;
    c->span_open = false;
    return end_event(c, c->span_ev);
}

bool schedule_fused(const spt_ctx* c) {
    if (c->cfg.flags & (SPT_FLAG_SPLIT_KERNELS | SPT_FLAG_SORTED_RAYS)) return false;
    if (c->fused_override >= 0) return c->fused_override != 0;
    return c->n_nodes == 0;
}

constexpr uint32_t kPersistentMaxFrames = 1024;

bool schedule_persistent(const spt_ctx* c, uint32_t n_frames) {
    if (c->cfg.max_bounces == 0) return false;
    if (c->cfg.flags & (SPT_FLAG_SPLIT_KERNELS | SPT_FLAG_WAVEFRONT | SPT_FLAG_SORTED_RAYS)) return false;
    if (c->persistent_override >= 0) return c->persistent_override != 0;
    // measured: C2 flat 18.5 -> 40+ Gsamples/s, C4 BVH 2.02 -> 2.34, C5 BVH even
    return n_frames >= SPT_PERSISTENT_MIN_FRAMES;
}

// calls of fewer frames: one persistent k_frame launch per frame (same conditions otherwise)
bool schedule_frame(const spt_ctx* c) {
    if (c->cfg.max_bounces == 0) return false;
    if (c->cfg.flags & (SPT_FLAG_SPLIT_KERNELS | SPT_FLAG_WAVEFRONT | SPT_FLAG_SORTED_RAYS)) return false;
    if (c->frame_override >= 0) return c->frame_override != 0;
    if (c->persistent_override >= 0) return c->persistent_override != 0;
    return true;
}

uint32_t schedule_tail(const spt_ctx* c) {
    if (c->tail_override) return c->tail_override;
    return c->n_nodes == 0 ? 3u : kMaxBounces;
}

// persistent launches use one zeroed set of work heads and zero the other for the next launch
void next_work_set(spt_ctx* c, PassParams& p) {
    p.work = c->work + c->work_parity * kWorkWords;
    p.work_next = c->work + (c->work_parity ^ 1u) * kWorkWords;
    c->work_parity ^= 1u;
}

// The run-time specialized kernels' key of the ctx's flat scene: its shape and, once configured, the
// launch configuration (spt_kernels.h jit_config_key).
static uint64_t flat_jit_key(const spt_ctx* c) {
    const uint64_t shape = flat_shape_key(c->flat_ends, c->n_prims, c->flat_rect, c->flat_pairs, c->flat_ranges);
    if (!c->configured) return shape;
    const uint32_t flags = (c->cfg.flags & ~spt::kFlagFastDiv) | (c->fast_div ? spt::kFlagFastDiv : 0u);
    return jit_config_key(shape, c->cfg.max_bounces, c->cfg.rr_depth, c->env.sky_enabled ? 1u : 0u, flags, c->has_camera);
}

// The NEE kernels run: the flag is set AND the scene has an emitter to sample (launch_paths / launch_frame
// select them from NeeParams::n_emit, which base_params sets from this)
// the sphere records of an emitter table (DevEmitter base[3] == 2)
static uint32_t sphere_emitters(const std::vector<DevEmitter>& emit) {
    uint32_t k = 0;
    for (const DevEmitter& e : emit) {
        uint32_t kind;
        std::memcpy(&kind, &e.base[3], 4);
        k += kind == 2u ? 1u : 0u;
    }
    return k;
}
static bool nee_active(const spt_ctx* c) { return c->configured && (c->cfg.flags & SPT_FLAG_NEE) && c->n_emit != 0u; }

// How far from the origin, per coordinate, the ctx's camera starts its rays (0 without one: the reference's
// pinhole at the origin): |origin| and, with a lens, the aperture around it
static float camera_reach(const spt_ctx* c) {
    if (!c->has_camera) return 0.0f;
    float r = 0.0f;
    for (int k = 0; k < 3; ++k) r = std::max(r, std::fabs(c->camera.origin[k]));
    return c->has_lens ? r + 2.0f * c->lens.radius : r;
}

// PassParams::cam_mode of the ctx's camera (has_camera)
static uint32_t camera_mode(const spt_ctx* c) {
    return ((c->camera.flags & SPT_CAMERA_JITTER) ? kCamJitter : kCamPosed) | (c->has_lens ? kCamLens : 0u);
}
// A lens's (a, b, f) on a camera: a = radius / |u|, b = radius / |v| in double, rounded once (a vanishing
// axis gives 0: the aperture has no extent along it)
static CameraLens lens_scalars(const spt_camera& cam, const spt_lens& lens) {
    auto len = [](const float v[3]) {
        return std::sqrt(((double)v[0] * v[0] + (double)v[1] * v[1]) + (double)v[2] * v[2]);
    };
    const double lu = len(cam.u), lv = len(cam.v);
    return CameraLens{lu > 0.0 ? (float)((double)lens.radius / lu) : 0.0f,
                      lv > 0.0 ? (float)((double)lens.radius / lv) : 0.0f, lens.focus_distance};
}
// Rewrite the camera's device record — (origin, mode), (u, a), (v, b), (w, f) — from the ctx's camera and
// lens; a launch in flight reads the old one, so the stream is drained first
static int write_camera_record(spt_ctx* c) {
    SPT_HIP(c, hipSetDevice(c->device));
    SPT_HIP(c, hipStreamSynchronize(on_stream(c)));
    if (const int rc = ensure_buf(c, c->d_camera, 4, "spt_set_camera"); rc != SPT_OK) return rc;
    const spt_camera& cam = c->camera;
    const CameraLens l = c->has_lens ? lens_scalars(cam, c->lens) : CameraLens{0.0f, 0.0f, 0.0f};
    const uint32_t mode = camera_mode(c);
    float4 rec[4] = {make_float4(cam.origin[0], cam.origin[1], cam.origin[2], 0.0f),
                     make_float4(cam.u[0], cam.u[1], cam.u[2], l.a), make_float4(cam.v[0], cam.v[1], cam.v[2], l.b),
                     make_float4(cam.w[0], cam.w[1], cam.w[2], l.f)};
    std::memcpy(&rec[0].w, &mode, sizeof(mode));
    SPT_HIP(c, hipMemcpy(c->d_camera, rec, sizeof(rec), hipMemcpyHostToDevice));
    return SPT_OK;
}

// the ctx may run wide launches (spt_launch_plan.h wide_possible): their kernel is compiled with the others
static bool wide_possible_ctx(const spt_ctx* c) {
    return c->view_cache >= 0 && c->px_shift == 0u && wide_possible(c->wide_chunks, c->pixels, c->cfg.shard_count, c->cu_count);
}

// Start compiling a configured flat scene's specialized kernels in the background (a new shape or a new
// configuration): frames rendered before they are ready run the generic kernels.
static void prefetch_flat(const spt_ctx* c) {
    if (!(c->has_scene && c->configured && c->n_prims && c->n_nodes == 0 && c->specialize == 0)) return;
    const uint64_t key = flat_jit_key(c);
    const JitFormList forms = jit_kinds_of_scene(nee_active(c), c->d_env ? 1 : 0, wide_possible_ctx(c));
    for (int i = 0; i < forms.n; ++i) jit_prefetch(forms.f[i], key);
}

PassParams base_params(spt_ctx* c) {
    PassParams p{};
    p.prims = c->d_prims;
    p.mats = c->d_mats;
    p.nodes = c->d_nodes;
    p.n_prims = c->n_prims;
    p.n_mats = c->n_mats;
    p.n_nodes = c->n_nodes;
    p.n_dev_nodes = c->n_dev_nodes;
    p.sky_enabled = c->env.sky_enabled ? 1u : 0u;
    p.flags = (c->cfg.flags & ~spt::kFlagFastDiv) | (c->fast_div ? spt::kFlagFastDiv : 0u);
    p.flat_ends = c->flat_ends;
    // flat scenes: their shape's kernels compiled at run time (spt_jit.hip), unless tuned off
    for (int a = 0; a < 3; ++a) {  // sorted ray queues: an 8 x 8 x 8 grid over the scene bounds
        p.bin_lo[a] = c->scene_lo[a];
        const float ext = c->scene_hi[a] - c->scene_lo[a];
        p.bin_scale[a] = ext > 0.0f ? 8.0f / ext : 0.0f;
    }
    p.ray_keys = c->ray_keys;
    p.ray_perm = c->ray_perm;
    p.ray_bins = c->ray_bins;
    p.ray_cursor = c->ray_cursor;
    p.jit_shape = (c->n_prims && c->n_nodes == 0 && c->specialize >= 0) ? flat_jit_key(c) : 0ull;
    p.jit_wait = c->specialize > 0 ? 1u : 0u;
    p.horizon = make_float4(c->env.horizon[0], c->env.horizon[1], c->env.horizon[2], 0.0f);
    p.zenith = make_float4(c->env.zenith[0], c->env.zenith[1], c->env.zenith[2], 0.0f);
    p.env = c->d_env;
    p.env_w = c->env_w;
    p.env_h = c->env_h;
    p.width = c->cfg.width;
    p.height = c->cfg.height;
    p.shard_rank = c->cfg.shard_rank;
    p.shard_count = c->cfg.shard_count;
    p.shard_pixels = c->pixels;
    // CPUPathTracer.cpp:53-54, 65
    p.inv_h = 1.0f / (float)c->cfg.height;
    p.inv_w = 1.0f / (float)c->cfg.width;
    p.aspect = (float)c->cfg.width / (float)c->cfg.height;
    p.max_bounces = c->cfg.max_bounces;
    p.rr_depth = c->cfg.rr_depth;
    p.n_sub = c->n_sub;
    p.sub_cap = c->sub_cap;
    for (int k = 0; k < 2; ++k) p.q[k] = QueueBufs{c->q_o[k], c->q_d[k], c->q_t[k]};
    p.hit = c->hit;
    p.radiance = c->radiance;
    p.accum = c->accum;
    p.counts = c->counts;
    p.totals = c->totals;
    p.cu_count = c->cu_count;
    // (auto: 4 for BVH scenes of <= 256 K primitives — C4 +1.3 %, C4 NEE +1.6 % over 2; 6: +1.5 %, 8: +0.6 % —
    // 2 otherwise: the C2 1/8 shard -5 % at 4, C5 -0.4 %; profiles/r06_t_ab_chunks_per_wave.txt)
    p.chunks_per_wave = c->chunks_per_wave ? c->chunks_per_wave
                                           : ((c->n_nodes != 0 && c->n_prims <= 256u * 1024u) ? 4u : 2u);
    p.px_shift = c->px_shift;
    p.stack = c->bvh_stack;
    p.stack_need = c->bvh_stack_need;
    p.stack_stride = c->bvh_stack_stride;
    p.stack_tb = c->bvh_stack_tb;
    // NEE only with the flag and something to sample (otherwise the oracle's integrator is the plain one)
    p.nee = NeeParams{c->d_emit, nee_active(c) ? c->n_emit : 0u, c->n_emit_spheres};
    if (c->has_camera) {
        p.cam_mode = camera_mode(c);
        p.cam_pose = c->d_camera;
    }
    p.bsdf = c->bsdf ? 1u : 0u;
    return p;
}

// The model word of a material (spt_device.h model_kind): +0.0f DIFFUSE, -fuzz METAL, ior DIELECTRIC.
float model_word(const spt_material_model& m) {
    if (m.kind == SPT_MAT_METAL) return -std::fabs(m.param);  // (a fuzz of -0.0f is a mirror too, not word 0)
    return m.kind == SPT_MAT_DIELECTRIC ? m.param : 0.0f;
}
// nullptr: valid
const char* model_error(const spt_material_model& m) {
    if (m.reserved[0] | m.reserved[1]) return "material model: reserved must be 0";
    if (!std::isfinite(m.param)) return "material model: non-finite parameter";
    if (m.kind == SPT_MAT_DIFFUSE) return m.param == 0.0f ? nullptr : "material model: a DIFFUSE parameter must be 0";
    if (m.kind == SPT_MAT_METAL) return m.param >= 0.0f && m.param <= 1.0f ? nullptr : "material model: fuzz outside [0, 1]";
    if (m.kind == SPT_MAT_DIELECTRIC) return m.param > 0.0f ? nullptr : "material model: index of refraction not > 0";
    return "material model: unknown kind";
}
// Upload the scene's device materials with the models' words (c->h_models; empty: none) and set c->bsdf.
// The caller has synchronized the stream.
int upload_materials(spt_ctx* c) {
    std::vector<DevMaterial> dm = c->h_dm;
    bool bsdf = false;
    if (!c->h_models.empty())
        for (size_t i = 0; i < dm.size(); ++i) {
            const spt_material_model& m = c->h_models[c->h_dev_mat[i]];
            dm[i].albedo[3] = model_word(m);
            bsdf = bsdf || m.kind != SPT_MAT_DIFFUSE;
        }
    SPT_HIP(c, hipMemcpy(c->d_mats, dm.data(), sizeof(DevMaterial) * dm.size(), hipMemcpyHostToDevice));
    c->bsdf = bsdf;
    return SPT_OK;
}


}  // namespace

extern "C" {

int spt_abi_version(void) { return SPT_ABI_VERSION; }

int spt_device_count(int* count) {
    if (!count) return SPT_ERR_INVALID;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
    *count = n;
    return SPT_OK;
}

int spt_create(spt_ctx** out, int device_id) {
    if (!out) return SPT_ERR_INVALID;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return SPT_ERR_NO_DEVICE;
    if (device_id < 0 || device_id >= n) return SPT_ERR_NO_DEVICE;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device_id) != hipSuccess) return SPT_ERR_NO_DEVICE;
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return SPT_ERR_NO_DEVICE;  // built for gfx950 only
    spt_ctx* c = new spt_ctx();
    c->device = device_id;
    c->cu_count = (uint32_t)std::max(prop.multiProcessorCount, 1);
    // Block-private sub-queues: 12 per CU (two rounds of 6 resident 256-thread shade blocks) measured
    // best on C2 among 4/6/8/12 per CU (scripts/gpu_sweep.sh).
    c->n_sub = c->cu_count * 12u;
    if (hipSetDevice(device_id) != hipSuccess || hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking) != hipSuccess ||
        !c->counts.alloc((size_t)2 * (kMaxBounces + 1) * c->n_sub) || !c->totals.alloc(kTotals) ||
        // (work heads: the ctx stream's two sets, then two per view half)
        !c->work.alloc(6 * kWorkWords) ||
        hipMemset(c->work, 0, sizeof(uint32_t) * 6 * kWorkWords) != hipSuccess ||
        hipStreamCreateWithFlags(&c->half[0].stream, hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithFlags(&c->half[1].stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&c->half[0].done, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->half[1].done, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->fork_ev, hipEventDisableTiming) != hipSuccess ||
        hipMemset(c->totals, 0, sizeof(unsigned long long) * kTotals) != hipSuccess ||
        hipMemset(c->counts, 0, sizeof(uint32_t) * 2 * (kMaxBounces + 1) * c->n_sub) != hipSuccess) {
        spt_destroy(c);
        return SPT_ERR_HIP;
    }
    for (uint32_t h = 0; h < 2u; ++h) c->half[h].work = c->work + (2u + 2u * h) * kWorkWords;
    on_stream(c) = c->own_stream;
    *out = c;
    return SPT_OK;
}

void spt_destroy(spt_ctx* c) {
    if (!c) return;
    if (c->device >= 0) (void)hipSetDevice(c->device);
    if (on_stream(c)) (void)hipStreamSynchronize(on_stream(c));
    for (ViewHalf& h : c->half)  // (joined into the ctx stream; a failed call may have left one unjoined)
        if (h.stream) (void)hipStreamSynchronize(h.stream);
    for (auto& e : c->pending) c->free_events.push_back(e);
    if (c->span_open) c->free_events.push_back(c->span_ev);
    for (auto& e : c->free_events) {
        if (e.a) (void)hipEventDestroy(e.a);
        if (e.b) (void)hipEventDestroy(e.b);
        if (e.a2) (void)hipEventDestroy(e.a2);
        if (e.b2) (void)hipEventDestroy(e.b2);
    }
    free_buffers(c);
    free_scene(c);
    free_comm(c);
    static_cast<OwnMem&>(*c) = {};  // (all device memory goes here, before the streams: `delete` finds the records empty)
    if (c->out_host) (void)hipHostUnregister(c->out_host);
    for (ViewHalf& h : c->half) {
        if (h.done) (void)hipEventDestroy(h.done);
        if (h.stream) (void)hipStreamDestroy(h.stream);
    }
    if (c->fork_ev) (void)hipEventDestroy(c->fork_ev);
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    delete c;
}

const char* spt_last_error(const spt_ctx* c) { return c ? c->err.c_str() : "null context"; }

int spt_set_stream(spt_ctx* c, void* hip_stream) {
    if (!c) return SPT_ERR_INVALID;
    SPT_HIP(c, hipSetDevice(c->device));
    SPT_HIP(c, hipStreamSynchronize(on_stream(c)));
    on_stream(c) = hip_stream ? (hipStream_t)hip_stream : c->own_stream;
    return SPT_OK;
}

int spt_set_scene(spt_ctx* c, const spt_prim* prims, uint32_t n_prims, const spt_material* mats, uint32_t n_mats,
                  const spt_env* env) {
    if (!c) return SPT_ERR_INVALID;
    if ((n_prims && !prims) || !mats || n_mats == 0 || !env) return fail(c, SPT_ERR_INVALID, "spt_set_scene: null array");
    SPT_HIP(c, hipSetDevice(c->device));
    std::vector<spt_prim> keep_prims(prims, prims + n_prims);  // (prims may alias c->h_prims)
    std::vector<spt_material> keep_mats(mats, mats + n_mats);
    // Flat scenes keep their records in LDS during shading (spt_kernels.hip): compact the materials
    // to the <= kFlatSceneMax ones the primitives use, in order of first use.
    std::vector<spt_prim> remapped;
    std::vector<spt_material> used_mats;
    std::vector<uint32_t> dev_mat;  // the caller's material behind each device material (spt_set_material_models)
    if (n_prims <= kFlatSceneMax) {
        std::vector<uint32_t> map(n_mats, 0xffffffffu);
        remapped.assign(prims, prims + n_prims);
        for (auto& p : remapped) {
            if (p.material >= n_mats) return fail(c, SPT_ERR_INVALID, "primitive material index out of range");
            if (map[p.material] == 0xffffffffu) {
                map[p.material] = (uint32_t)used_mats.size();
                used_mats.push_back(mats[p.material]);
                dev_mat.push_back(p.material);
            }
            p.material = map[p.material];
        }
        if (used_mats.empty()) {
            used_mats.push_back(mats[0]);
            dev_mat.push_back(0u);
        }
        prims = remapped.data();
        mats = used_mats.data();
        n_mats = (uint32_t)used_mats.size();
    }
    std::vector<DevPrim> dp;
    const char* msg = nullptr;
    if (!prepare_prims(prims, n_prims, n_mats, dp, &msg)) return fail(c, SPT_ERR_INVALID, msg);
    const bool fast_div = fast_division_ok(prims, n_prims, dp);  // before build_bvh reorders dp
    // (a flat scene's: of the materials its primitives use, so an edit that brings another one in re-derives it)
    const bool flat_ranges = n_prims && n_prims <= kFlatSceneMax && flat_ranges_ok(prims, n_prims, mats, n_mats, dp);
    std::vector<DevMaterial> dm;
    prepare_materials(mats, n_mats, dm);
    std::vector<DevEmitter> emit;  // SPT_FLAG_NEE's emitters (built for every scene: the flag may come later)
    build_emitters(prims, n_prims, mats, emit);
    std::vector<BvhNode> nodes;
    if (n_prims >= (1u << 27)) return fail(c, SPT_ERR_CAPACITY, "scene too large (>= 2^27 primitives)");
    if (n_prims > kFlatSceneMax) {
        uint32_t max_leaf = bvh_max_leaf(n_prims);  // scene.h
        if (c->bvh_max_leaf >= 1 && c->bvh_max_leaf <= kBvhMaxLeaf) max_leaf = c->bvh_max_leaf;  // spt_tuning
        build_bvh(prims, dp, nodes, max_leaf, c->bvh_bins, camera_reach(c));
    }
    // the device traverses the W-wide collapse of the binary SAH tree (device_tree); a tree too deep for
    // the traversal stacks is refused before anything of the current scene is freed
    const DevTree tree = device_tree(nodes);
    const uint32_t stack_need = tree.stack_need;
    const uint32_t stack_tb = tree.stack_tb;
    if (stack_need > kBvhStackEntries)
        return fail(c, SPT_ERR_CAPACITY, "spt_set_scene: the BVH needs " + std::to_string(stack_need) +
                                             " traversal stack entries (at most " + std::to_string(kBvhStackEntries) + ")");
    SPT_HIP(c, hipStreamSynchronize(on_stream(c)));
    free_scene(c);
    uint32_t flat_ends = 0, flat_rect = 0, flat_pairs = 0;
    if (n_prims && n_prims <= kFlatSceneMax) {  // flat: the originals, then the kind-major copy
        std::vector<DevPrim> sorted;
        uint32_t ends[kFlatKinds - 1];
        sort_flat_by_kind(dp, sorted, ends);
        for (uint32_t g = 0; g + 1 < kFlatKinds; ++g) flat_ends |= ends[g] << (6 * g);
        flat_rect = flat_rect_bits(sorted, ends);
        flat_pairs = flat_wall_pairs(sorted, ends, flat_rect);  // (reorders the axis groups: pairs first)
        dp.insert(dp.end(), sorted.begin(), sorted.end());
    }
    if (dev_mat.empty())  // (a BVH scene keeps the caller's materials as they are)
        for (uint32_t i = 0; i < n_mats; ++i) dev_mat.push_back(i);
    const void* node_data = tree.bytes.data();  // quantized (scene.h), exact decode on the device
    const uint64_t node_bytes = tree.bytes.size();
    // every resident lane's traversal stack (8 waves x 4 SIMDs per CU), as deep as the tree needs
    const uint32_t stride = nodes.empty() ? 0u : bvh_stack_stride(stack_need);
    // (a failure from here on leaves has_scene false, free_scene's: nothing reads a partly uploaded scene, and
    // the next spt_set_scene frees it)
    if (!c->d_prims.alloc(float4s<DevPrim>(dp.size())) || !c->d_mats.alloc(float4s<DevMaterial>(n_mats)) ||
        !c->d_mat_map.alloc(dev_mat.size()) || !c->d_emit.alloc(float4s<DevEmitter>(emit.size())) ||
        !c->d_nodes.alloc(node_bytes / sizeof(float4)) ||
        !c->bvh_stack.alloc((size_t)kBvhStackEntryBytes * stride * 64u * kMaxResidentWaves * c->cu_count))
        return fail(c, SPT_ERR_HIP, "spt_set_scene: allocation failed");
    c->bvh_stack_stride = stride;
    if (n_prims) SPT_HIP(c, hipMemcpy(c->d_prims, dp.data(), sizeof(DevPrim) * dp.size(), hipMemcpyHostToDevice));
    SPT_HIP(c, hipMemcpy(c->d_mats, dm.data(), sizeof(DevMaterial) * n_mats, hipMemcpyHostToDevice));
    SPT_HIP(c, hipMemcpy(c->d_mat_map, dev_mat.data(), sizeof(uint32_t) * dev_mat.size(), hipMemcpyHostToDevice));
    if (!emit.empty()) SPT_HIP(c, hipMemcpy(c->d_emit, emit.data(), sizeof(DevEmitter) * emit.size(), hipMemcpyHostToDevice));
    if (node_bytes) SPT_HIP(c, hipMemcpy(c->d_nodes, node_data, node_bytes, hipMemcpyHostToDevice));
    c->n_prims = n_prims;
    c->n_mats = n_mats;
    c->n_emit = (uint32_t)emit.size();
    c->n_emit_spheres = sphere_emitters(emit);
    c->n_nodes = (uint32_t)nodes.size();
    c->n_dev_nodes = (uint32_t)(node_bytes / kDevNodeBytes);
    c->pad_reach = camera_reach(c);
    c->scene_mag = scene_magnitude(prims, n_prims);
    c->bvh_stack_need = stack_need;
    c->bvh_stack_tb = stack_tb;
    c->env = *env;
    c->has_scene = true;
    c->fast_div = fast_div;
    c->flat_ranges = flat_ranges;
    c->flat_ends = flat_ends;
    c->flat_rect = flat_rect;
    c->flat_pairs = flat_pairs;
    c->h_prims.swap(keep_prims);
    c->h_mats.swap(keep_mats);
    c->h_dev_mat.swap(dev_mat);
    c->h_dm.swap(dm);
    c->h_models.clear();  // a new scene's materials are all DIFFUSE
    c->bsdf = false;
    if (n_prims > kFlatSceneMax) {  // what spt_update_prims refits
        c->h_dp = dp;
        c->h_nodes = nodes;
        c->h_pos.assign(n_prims, 0u);
        for (uint32_t i = 0; i < n_prims; ++i) {
            uint32_t orig;
            std::memcpy(&orig, &dp[i].b[3], sizeof orig);  // DevPrim b.w: the original index's bits
            c->h_pos[orig] = i;
        }
    } else {
        c->h_dp.clear();
        c->h_nodes.clear();
        c->h_pos.clear();
    }
    if (!nodes.empty()) {  // the root's bounds: the sorted schedule's binning grid
        for (int a = 0; a < 3; ++a) {
            c->scene_lo[a] = nodes[0].lo[a];
            c->scene_hi[a] = nodes[0].hi[a];
        }
    }
    c->scene_bytes = sizeof(DevPrim) * (uint64_t)dp.size() + node_bytes + sizeof(DevMaterial) * (uint64_t)n_mats +
                     sizeof(DevEmitter) * (uint64_t)emit.size();
    c->stack_bytes = (uint64_t)kBvhStackEntryBytes * c->bvh_stack_stride * 64u * kMaxResidentWaves * c->cu_count;
    // a flat scene of a new shape: its specialized kernels start compiling now, off the render thread
    // (rebuild_scene -> here); frames rendered before they are ready run the generic kernels
    prefetch_flat(c);
    // scene change -> m_frameCount = 0 (CPUPathTracer.cpp:122-131)
    if (c->configured) return spt_reset(c);
    return SPT_OK;
}

// spt_update_prims; edit false: no primitive changes (n == 0) and the caller invalidates and resets — a BVH
// scene's boxes padded again for the ctx's camera (repad_for_camera)
static int refit_scene(spt_ctx* c, const uint32_t* indices, const spt_prim* prims, uint32_t n, bool edit) {
    if (!c) return SPT_ERR_INVALID;
    if (!c->has_scene) return fail(c, SPT_ERR_NO_SCENE, "spt_update_prims before spt_set_scene");
    if (n && (!indices || !prims)) return fail(c, SPT_ERR_INVALID, "spt_update_prims: null array");
    const uint32_t total = (uint32_t)c->h_prims.size();
    std::vector<DevPrim> upd;
    const char* msg = nullptr;
    if (!prepare_prims(prims, n, (uint32_t)c->h_mats.size(), upd, &msg)) return fail(c, SPT_ERR_INVALID, msg);
    for (uint32_t j = 0; j < n; ++j)
        if (indices[j] >= total) return fail(c, SPT_ERR_INVALID, "spt_update_prims: index out of range");
    if (edit) c->derived.drop(Change::Prims);
    // the edits are staged and committed to the host mirror only once the device holds them, so a
    // failed call leaves the ctx's scene as it was
    std::vector<spt_prim> all = c->h_prims;
    for (uint32_t j = 0; j < n; ++j) all[indices[j]] = prims[j];
    if (c->h_nodes.empty()) {  // flat scene: its records are a few hundred bytes, re-prepare them all
        const std::vector<spt_material> mats = c->h_mats;
        const std::vector<spt_material_model> models = c->h_models;  // (they belong to the materials: kept)
        const spt_env env = c->env;
        const int rc = spt_set_scene(c, all.data(), total, mats.data(), (uint32_t)mats.size(), &env);
        if (rc != SPT_OK || models.empty()) return rc;
        return spt_set_material_models(c, models.data(), (uint32_t)models.size());
    }
    // BVH scene: the changed records at their device positions, the tree refitted (same topology:
    // no rebuild), the 4-wide collapse and its quantization redone, the node array re-uploaded
    std::vector<DevPrim> dp = c->h_dp;
    std::vector<BvhNode> tree = c->h_nodes;
    uint32_t lo = UINT32_MAX, hi = 0;  // the device positions touched: uploaded as one range
    for (uint32_t j = 0; j < n; ++j) {
        DevPrim d = upd[j];
        std::memcpy(&d.b[3], &indices[j], sizeof(uint32_t));  // the original index stays the tie-break key
        const uint32_t at = c->h_pos[indices[j]];
        dp[at] = d;
        lo = std::min(lo, at);
        hi = std::max(hi, at);
    }
    const float reach = camera_reach(c);
    refit_bvh(all.data(), total, dp, tree, reach);
    std::vector<DevEmitter> emit;  // moved emitters move their samples
    build_emitters(all.data(), total, c->h_mats.data(), emit);
    const DevTree dtree = device_tree(tree);
    const uint32_t stack_need = dtree.stack_need;  // (the refit can change the collapse)
    if (stack_need > kBvhStackEntries)
        return fail(c, SPT_ERR_CAPACITY, "spt_update_prims: the refitted BVH needs " + std::to_string(stack_need) +
                                             " traversal stack entries (at most " + std::to_string(kBvhStackEntries) + ")");
    const void* node_data = dtree.bytes.data();
    const uint64_t node_bytes = dtree.bytes.size();
    SPT_HIP(c, hipSetDevice(c->device));
    SPT_HIP(c, hipStreamSynchronize(on_stream(c)));
    // Every allocation the edit needs comes first — a grown node array (the 4-wide collapse opens the
    // largest children first, so refitted areas can change its node count), the emitter array, deeper
    // traversal stacks — and only once all of them have succeeded is anything copied or swapped in: a
    // failed call leaves the device scene, the stacks and their sizes exactly as they were.
    const uint32_t stride = bvh_stack_stride(stack_need);
    const size_t stack_bytes = (size_t)kBvhStackEntryBytes * stride * 64u * kMaxResidentWaves * c->cu_count;
    Dev<float4> grown_nodes, new_emit;  // (what is not swapped in goes when the call returns)
    Dev<uint8_t> grown_stack;
    const size_t node_elems = node_bytes / sizeof(float4);
    const bool emit_changed = emit.size() != c->n_emit;  // (an edit can make an emitter degenerate, or not)
    if ((node_elems > c->d_nodes.size() && !grown_nodes.alloc(node_elems)) ||
        (emit_changed && !new_emit.alloc(float4s<DevEmitter>(emit.size()))) ||
        (stride > c->bvh_stack_stride && !grown_stack.alloc(stack_bytes)))  // deeper than allocated
        return fail(c, SPT_ERR_HIP, "spt_update_prims: allocation failed");
    // the copies into the buffers that stay (new buffers are swapped in only after theirs succeeded)
    float4* nodes_dst = grown_nodes ? grown_nodes : c->d_nodes;
    float4* emit_dst = emit_changed ? new_emit : c->d_emit;
    hipError_t e = hipMemcpy(nodes_dst, node_data, node_bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess && !emit.empty()) e = hipMemcpy(emit_dst, emit.data(), sizeof(DevEmitter) * emit.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess && n)
        e = hipMemcpy(c->d_prims + 4u * lo, &dp[lo], sizeof(DevPrim) * (hi - lo + 1u), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        // a copy into the kept buffers may have landed partly: the device no longer matches the host
        // mirror, so the scene is dropped (the next render fails with SPT_ERR_NO_SCENE, not wrong bits)
        (void)hipGetLastError();
        free_scene(c);
        c->has_scene = false;
        return fail(c, SPT_ERR_HIP, std::string("spt_update_prims: upload failed: ") + hipGetErrorString(e));
    }
    if (grown_nodes) c->d_nodes.swap(grown_nodes);
    if (emit_changed) c->d_emit.swap(new_emit);
    c->n_emit = (uint32_t)emit.size();
    c->n_emit_spheres = sphere_emitters(emit);
    c->n_dev_nodes = (uint32_t)(node_bytes / kDevNodeBytes);
    if (grown_stack) {
        c->bvh_stack.swap(grown_stack);
        c->bvh_stack_stride = stride;
        c->stack_bytes = stack_bytes;
    }
    c->bvh_stack_need = stack_need;
    c->bvh_stack_tb = dtree.stack_tb;  // (the collapse can add nodes)
    c->pad_reach = reach;
    c->scene_mag = scene_magnitude(all.data(), total);
    c->h_prims.swap(all);
    c->h_dp.swap(dp);
    c->h_nodes.swap(tree);
    for (int a = 0; a < 3; ++a) {
        c->scene_lo[a] = c->h_nodes[0].lo[a];
        c->scene_hi[a] = c->h_nodes[0].hi[a];
    }
    // scene change -> m_frameCount = 0 (CPUPathTracer.cpp:122-131)
    if (edit && c->configured) return spt_reset(c);
    return SPT_OK;
}

int spt_update_prims(spt_ctx* c, const uint32_t* indices, const spt_prim* prims, uint32_t n) {
    return refit_scene(c, indices, prims, n, true);
}

int spt_configure(spt_ctx* c, const spt_config* cfg) {
    if (!c || !cfg) return SPT_ERR_INVALID;
    if (cfg->width == 0 || cfg->height == 0) return fail(c, SPT_ERR_INVALID, "width and height must be > 0");
    if (cfg->max_bounces > kMaxBounces) return fail(c, SPT_ERR_INVALID, "max_bounces > 32");
    if (cfg->shard_count == 0 || cfg->shard_rank >= cfg->shard_count)
        return fail(c, SPT_ERR_INVALID, "shard_rank must be < shard_count");
    if ((uint64_t)cfg->width * cfg->height >= (1ull << 31)) return fail(c, SPT_ERR_INVALID, "image too large");
    SPT_HIP(c, hipSetDevice(c->device));
    SPT_HIP(c, hipStreamSynchronize(on_stream(c)));
    const uint32_t rows = cfg->shard_rank < cfg->height
                              ? (cfg->height - cfg->shard_rank + cfg->shard_count - 1) / cfg->shard_count
                              : 0u;
    const uint32_t pixels = rows * cfg->width;
    uint32_t fpp = cfg->frames_in_flight;
    if (fpp == 0) {
        // auto: about 2^24 paths per pass (8 frames at 1920x1080): fewer, fuller launches
        const uint32_t target = 1u << 24;
        fpp = pixels ? std::max(1u, std::min(256u, target / std::max(pixels, 1u))) : 1u;
    }
    if ((uint64_t)fpp * pixels >= (1ull << 31)) return fail(c, SPT_ERR_INVALID, "frames_in_flight * pixels too large");
    const uint32_t cap = sub_capacity((uint64_t)fpp * pixels, c->n_sub);
    const bool realloc = !c->configured || pixels != c->pixels || fpp != c->frames_per_pass || c->sub_alloc != c->n_sub;
    c->cfg = *cfg;
    c->accum_shared = false;  // (a pointer handed out before is no longer valid: spt.h)
    c->rows = rows;
    c->pixels = pixels;
    c->frames_per_pass = fpp;
    c->sub_cap = cap;
    const size_t qn = (size_t)cap * c->n_sub;
    bool ok = true;
    if (realloc) {
        // not configured until every buffer of the new size exists: a failed allocation leaves a ctx that
        // answers SPT_ERR_NOT_CONFIGURED, never one whose next launch runs over buffers that are not there
        c->configured = false;
        free_buffers(c);
        c->sub_alloc = c->n_sub;
        const size_t px = std::max<size_t>(pixels, 1);
        for (int k = 0; k < 2; ++k) ok = ok && c->q_o[k].alloc(qn) && c->q_d[k].alloc(qn) && c->q_t[k].alloc(qn);
        ok = ok && c->hit.alloc(qn) && c->radiance.alloc(qn ? (size_t)fpp * pixels : 0u) && c->accum.alloc(px) &&
             c->hit_cache.alloc(px) && c->chunk_cost.alloc(px) && c->chunk_order.alloc(px);
        if (kFrameHitCache >= 2)
            ok = ok && c->live_rec.alloc(px) && c->sky_pix.alloc(px) && c->list_counts.alloc(2 + (pixels + kBlock - 1) / kBlock);
        ok = ok && c->resolved.alloc(px);
    }
    c->derived.drop(Change::Configuration);
    if ((cfg->flags & SPT_FLAG_SORTED_RAYS) && qn && !c->ray_perm)  // the sorted schedule's buffers
        ok = ok && c->ray_keys.alloc(qn) && c->ray_perm.alloc(qn) && c->ray_bins.alloc(4096) && c->ray_cursor.alloc(4097) &&
             hipMemset(c->ray_bins, 0, sizeof(uint32_t) * 4096) == hipSuccess;
    if (!ok) {  // (whichever it was: nothing of a configuration is left)
        c->configured = false;
        free_buffers(c);
        return fail(c, SPT_ERR_HIP, "spt_configure: allocation failed");
    }
    c->configured = true;
    prefetch_flat(c);  // (a flat scene's kernels are compiled for the configuration too)
    // settings dirty / resize -> m_frameCount = 0 and a zeroed accumulation (CPUPathTracer.cpp:132-154)
    return spt_reset(c);
}

int spt_reset(spt_ctx* c) {
    if (!c) return SPT_ERR_INVALID;
    if (!c->configured) return fail(c, SPT_ERR_NOT_CONFIGURED, "spt_reset before spt_configure");
    SPT_HIP(c, hipSetDevice(c->device));
    SPT_HIP(c, hipMemsetAsync(c->accum, 0, sizeof(float4) * std::max<size_t>(c->pixels, 1), on_stream(c)));
    c->frame_count = 0;
    c->noise_batches = c->noise_frames = 0;  // (the noise estimate restarts with the accumulation)
    c->noise_W = 0.0f;
    c->noise_metered = false;
    return SPT_OK;
}

int spt_get_frame_count(const spt_ctx* c, uint32_t* fc) {
    if (!c || !fc) return SPT_ERR_INVALID;
    *fc = c->frame_count;
    return SPT_OK;
}

// Build flat k_paths' view lists behind the persistent launch just enqueued (stream order) and read the
// two counts back: they size the next launches' plans and grids. This waits for that launch, once per
// view — on the first persistent call after a change only, as k_frame's lists do below. A failed
// allocation is no error: the launches keep computing bounce 0 themselves.
static int build_view_lists(spt_ctx* c, const PassParams& p) {
    const size_t pixels = std::max<size_t>(c->pixels, 1);
    const size_t blocks = (pixels + kBlock - 1) / kBlock;
    if (!c->view_live.ensure(3 * pixels) || !c->view_const.ensure(pixels) || !c->view_counts.ensure(2 + blocks)) {
        c->derived.produced(kViewNoMemory);  // (the launches never take lists while it is set: a part of them may stay)
        return SPT_OK;
    }
    launch_view_lists(p, c->view_live, c->view_const, c->view_counts, c->view_counts + 2, on_stream(c));
    SPT_HIP(c, hipGetLastError());
    SPT_HIP(c, hipMemcpyAsync(c->view_n, c->view_counts, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, on_stream(c)));
    SPT_HIP(c, hipStreamSynchronize(on_stream(c)));
    c->derived.produced_view_lists();
    return SPT_OK;
}

// ---- split launches: a view's lists in two halves on two streams (spt_launch_plan.h make_view_split) ----
// Consecutive k_paths launches in one stream leave wave slots idle: when launch k's waves run out of
// chunks, launch k+1 is enqueued but stream order keeps it out until the last wave of k has left. A pixel's
// frames must be added in order, but two launches over disjoint pixels need no order at all: half A's
// launches follow each other on half[0].stream, half B's on half[1].stream, and nothing waits across the
// halves, so each launch's blocks move in as the waves of the launch before it leave.
// Ordering against everything else is by events, never by a host wait:
//   fork  a split launch that finds the ctx stream dirty (something ran on it, or drained it to change what
//         a launch reads, since the last fork: on_stream) makes both half streams wait on it first;
//   join  a call that launched halves makes the ctx stream wait on them before it returns, so whatever the
//         caller orders behind the call on its stream sees the finished render. The wait sits in the ctx
//         stream and does not hold the half streams back.
// Whether a call's launches are split is decided once per call (spt_launch_plan.h split_call_wanted), never
// per launch: a call never goes from split launches back to a whole one.

// The halves' cost and order buffers, allocated by the first split launch of a configuration: a half holds at
// most half the live list plus half a chunk, and its first tier at most a chunk per record. false: no memory
// (the launch runs unsplit).
static bool half_buffers(spt_ctx* c) {
    const size_t n = (size_t)c->pixels / 2u + 64u;
    for (auto& h : c->half_mem)
        if (!h.cost.ensure(n) || !h.order.ensure(n)) return false;
    return true;
}

// One persistent launch as two: `whole` is the view's lists, p the launch's parameters (its work heads and
// chunk buffers are replaced by each half's own). launched[h]: half h got a launch (an empty half gets none).
static int launch_paths_split(spt_ctx* c, PassParams p, const ViewPlan& whole, bool launched[2], int wide) {
    const ViewSplit sp = make_view_split(whole.n_live, whole.n_const, wide ? kWidePx : 1u << kMaxChunkShift);
    EventPair span_ev;
    if (c->profiling && c->span && begin_persistent(c, span_ev) != SPT_OK) return SPT_ERR_HIP;  // (the span's begin: ctx stream)
    if (c->stream_dirty || c->accum_shared) {  // fork
        SPT_HIP(c, hipEventRecord(c->fork_ev, c->user_stream));
        for (ViewHalf& h : c->half) SPT_HIP(c, hipStreamWaitEvent(h.stream, c->fork_ev, 0));
        c->stream_dirty = false;
    }
    // No small tail tiers under the split (unless spt_tuning.chunks_per_wave asks for them): the tiers square
    // off a launch's end at two and four times a 32-pixel chunk's drain per pixel, and here the other half's
    // next launch fills that end anyway. Measured: C2 +1.5 %, the N = 8 shard +2.3 % over
    // the split with both tiers. The live records left over by the first tier still go to the last tier.
    if (!c->chunks_per_wave) p.chunks_per_wave = 0u;
    const bool timed = c->profiling && !c->span;
    EventPair ev[2];
    int n_ev = 0;
    int rc = SPT_OK;
    for (uint32_t h = 0; h < 2u && rc == SPT_OK; ++h) {
        if (view_half_empty(sp, h)) continue;
        ViewHalf& vh = c->half[h];
        const ViewPlan view{whole.live + 3u * (size_t)sp.live_at[h], whole.constant + sp.const_at[h],
                            sp.live_at[h + 1] - sp.live_at[h], sp.const_at[h + 1] - sp.const_at[h], 0u};
        p.work = vh.work + vh.work_parity * kWorkWords;
        p.work_next = vh.work + (vh.work_parity ^ 1u) * kWorkWords;
        vh.work_parity ^= 1u;
        p.chunk_cost = c->half_mem[h].cost;
        p.chunk_order = c->half_mem[h].order;
        p.chunk_order_key = &c->derived.half_order_key[h];
        if (timed) {
            if (take_events(c, ev[n_ev], 4) != SPT_OK) return SPT_ERR_HIP;
            ++n_ev;
            if (hipEventRecord(ev[n_ev - 1].a, vh.stream) != hipSuccess) rc = fail(c, SPT_ERR_HIP, "k_paths (split): hipEventRecord");
        }
        c->last_specialized = launch_paths(p, c->counters, vh.stream, &view, h + 1u, wide, &c->last_view_wide);
        launched[h] = true;
        // a failed launch leaves no chunk order behind (a retry must not read an unsorted buffer)
        const hipError_t le = hipGetLastError();
        if (le != hipSuccess) {
            c->derived.half_order_key[h] = 0;
            rc = fail(c, SPT_ERR_HIP, std::string("k_paths (split): ") + hipGetErrorString(le));
        }
        if (timed && hipEventRecord(ev[n_ev - 1].b, vh.stream) != hipSuccess) rc = fail(c, SPT_ERR_HIP, "k_paths (split): hipEventRecord");
    }
    c->last_pairs = c->last_specialized ? flat_shape_pairs(p.jit_shape) : 0u;
    c->last_ranges = c->last_specialized && flat_ranges_baked(p.jit_shape);
    if (rc != SPT_OK) {
        for (int i = 0; i < n_ev; ++i) c->free_events.push_back(ev[i]);
        c->derived.half_order_key[0] = c->derived.half_order_key[1] = 0;
        return rc;
    }
    if (n_ev) {  // one persistent launch: the two pairs as one record
        if (n_ev == 2) {
            ev[0].a2 = ev[1].a;
            ev[0].b2 = ev[1].b;
        }
        c->pending.push_back(ev[0]);
        if (c->pending.size() >= 4096) return flush_events(c);
    }
    return SPT_OK;
}

// the join: the ctx stream waits on the halves launched since the last join (not through on_stream: the wait
// orders nothing a later fork would have to wait for). Every half is tried even if one fails.
static int join_halves(spt_ctx* c, bool launched[2]) {
    int rc = SPT_OK;
    for (uint32_t h = 0; h < 2u; ++h) {
        if (!launched[h]) continue;
        launched[h] = false;
        hipError_t e = hipEventRecord(c->half[h].done, c->half[h].stream);
        if (e == hipSuccess) e = hipStreamWaitEvent(c->user_stream, c->half[h].done, 0);
        if (e != hipSuccess) rc = fail(c, SPT_ERR_HIP, std::string("k_paths (split) join: ") + hipGetErrorString(e));
    }
    return rc;
}

// The persistent schedule's launches of one spt_render call: one per <= kPersistentMaxFrames frames, every
// path of the call, accumulated in frame order in-kernel (fewer, longer launches amortize each launch's
// tail). launched[]: the view halves with launches the ctx stream has not been joined with yet; whatever this
// returns, the caller joins them.
static int render_persistent(spt_ctx* c, PassParams& p, uint32_t first_frame, uint32_t n_frames, bool launched[2]) {
    uint32_t done = 0;
    while (done < n_frames) {
        // (a call whose launches over the view may be wide takes at most kWideMaxFrames frames per such launch:
        // the ring's lap byte; decided for the call, as the split is)
        const bool view_now = c->view_cache >= 0 && c->derived.valid(kViewLists) && view_lists_scene(p);
        const int wide = view_now ? wide_call(c->wide_chunks, wide_eligible(p), wide_first_tier(c->pixels, c->cu_count), c->view_n[0], n_frames) : 0;
        const uint32_t f = std::min(wide ? kWideMaxFrames : kPersistentMaxFrames, n_frames - done);
        p.first_frame = first_frame + done;
        p.n_frames = f;
        p.n_paths = f * c->pixels;
        // a flat scene's view lists, once they are built (below): the launch runs over them
        const bool view_scene = c->view_cache >= 0 && view_lists_scene(p);
        const ViewPlan view{c->view_live, c->view_const, c->view_n[0], c->view_n[1], 0u};
        const bool view_on = view_scene && c->derived.valid(kViewLists);
        // ... in two halves on two streams (the first persistent launch of a view stays whole on the ctx
        // stream: it builds the lists). Decided for the call, not for the launch: the same answer for every
        // launch of the call once the lists exist.
        if (view_on && split_call_wanted(c->split_streams, c->view_n[0], n_frames, kPersistentMaxFrames) && half_buffers(c)) {
            c->last_view_cached = c->last_view_split = true;
            const int rc = launch_paths_split(c, p, view, launched, wide);
            if (rc != SPT_OK) return rc;
            done += f;
            c->passes++;
            continue;
        }
        // a whole launch on the ctx stream: behind any halves still in flight (they write the same pixels)
        if (join_halves(c, launched) != SPT_OK) return SPT_ERR_HIP;
        c->last_view_split = false;
        EventPair ev;
        if (begin_persistent(c, ev) != SPT_OK) return SPT_ERR_HIP;
        next_work_set(c, p);
        p.chunk_cost = c->chunk_cost;
        p.chunk_order = c->chunk_order;
        p.chunk_order_key = &c->derived.chunk_order_key;
        c->last_specialized = launch_paths(p, c->counters, on_stream(c), view_on ? &view : nullptr, 0u, wide, &c->last_view_wide);
        c->last_pairs = c->last_specialized ? flat_shape_pairs(p.jit_shape) : 0u;
        c->last_ranges = c->last_specialized && flat_ranges_baked(p.jit_shape);
        c->last_view_cached = view_on;
        // a failed launch leaves no chunk order behind (a retry must not read an unsorted buffer)
        const hipError_t le = hipGetLastError();
        if (le != hipSuccess) c->derived.chunk_order_key = 0;
        if (end_persistent(c, ev) != SPT_OK) {
            c->derived.chunk_order_key = 0;
            return SPT_ERR_HIP;
        }
        SPT_HIP(c, le);
        const bool build = view_scene && !c->derived.valid(kViewLists) && !c->derived.valid(kViewNoMemory);
        if (build && build_view_lists(c, p) != SPT_OK) return SPT_ERR_HIP;
        done += f;
        c->passes++;
    }
    return SPT_OK;
}

int spt_render(spt_ctx* c, uint32_t first_frame, uint32_t n_frames) {
    if (!c) return SPT_ERR_INVALID;
    if (!c->has_scene) return fail(c, SPT_ERR_NO_SCENE, "Scene not set before rendering");  // CPUPathTracer.cpp:46
    if (!c->configured) return fail(c, SPT_ERR_NOT_CONFIGURED, "spt_render before spt_configure");
    if (c->sub_alloc != c->n_sub) return fail(c, SPT_ERR_NOT_CONFIGURED, "spt_set_tuning(subqueues) takes effect at spt_configure");
    SPT_HIP(c, hipSetDevice(c->device));
    if (c->pixels == 0 || n_frames == 0) {
        c->frame_count += n_frames;
        return SPT_OK;
    }
    PassParams p = base_params(c);
    uint32_t done = 0;
    if (schedule_persistent(c, n_frames)) {
        c->last_schedule = SPT_SCHEDULE_PERSISTENT;
        bool launched[2] = {false, false};
        const int rc = render_persistent(c, p, first_frame, n_frames, launched);
        const std::string err = c->err;
        const int joined = join_halves(c, launched);  // (also behind a failed launch: the ctx stream is never left unjoined)
        if (rc != SPT_OK) {
            c->err = err;  // (the launch's message, not the join's)
            return rc;
        }
        if (joined != SPT_OK) return joined;
        c->frames += n_frames;
        c->paths += (uint64_t)n_frames * c->pixels;
        c->frame_count += n_frames;
        return SPT_OK;
    }
    if (schedule_frame(c)) {
        c->last_schedule = SPT_SCHEDULE_FRAME;
        for (; done < n_frames; ++done) {  // stream order keeps the frames' accumulation order
            p.first_frame = first_frame + done;
            p.n_frames = 1;
            p.n_paths = c->pixels;
            EventPair ev;
            if (begin_persistent(c, ev) != SPT_OK) return SPT_ERR_HIP;
            next_work_set(c, p);
            p.hit_cache = c->hit_cache;
            p.live_rec = c->live_rec;
            p.sky_pix = c->sky_pix;
            p.list_counts = c->list_counts;
            // (a jittered or lens camera: hit_mode 0, the camera segment traced per frame; no cache, no lists, no wait)
            const bool jitter = cam_per_path(p.cam_mode) || p.bsdf != 0u;  // (and so do material models)
            p.hit_mode = frame_hit_mode(p, c->derived.valid(kCameraHits), c->derived.frame_lists());
            p.live_pixels = c->live_pixels;
            if (c->fuse_frames != 0.0f && done + 1u == n_frames) {  // the call's last frame resolves as it ends
                p.rgba = (uint32_t*)c->out_dev;
                p.rgba_frames = c->fuse_frames;
                p.rgba_exposure = c->fuse_exposure;
                c->fused = true;
            }
            c->last_specialized = launch_frame(p, c->counters, on_stream(c));
            c->last_pairs = c->last_specialized ? flat_shape_pairs(p.jit_shape) : 0u;
            c->last_ranges = false;  // (k_frame has no such forms)
            if (end_persistent(c, ev) != SPT_OK) return SPT_ERR_HIP;
            SPT_HIP(c, hipGetLastError());
            bool lists = c->derived.frame_lists();
            if (!jitter && !c->derived.valid(kCameraHits) && frame_lists_scene(p, c->counters)) {  // compacted once (stream order)
                launch_hit_lists(p, c->list_counts + 2, on_stream(c));
                SPT_HIP(c, hipGetLastError());
                // the live count sizes the next launches' grids: read back once per scene / configuration
                // (this waits for the frame just launched, ~0.1 ms, on the first frame after a change only)
                SPT_HIP(c, hipMemcpyAsync(&c->live_pixels, c->list_counts, sizeof(uint32_t), hipMemcpyDeviceToHost,
                                          on_stream(c)));
                SPT_HIP(c, hipStreamSynchronize(on_stream(c)));
                lists = c->pixels - c->live_pixels >= c->pixels / kFrameListsMinSkyDiv;
            }
            if (!jitter) c->derived.produced_camera_hits(lists);  // (stream order: the next launch reads what this one stored)
            c->passes++;
        }
        c->frames += n_frames;
        c->paths += (uint64_t)n_frames * c->pixels;
        c->frame_count += n_frames;
        return SPT_OK;
    }
    c->last_schedule = schedule_fused(c) ? SPT_SCHEDULE_FUSED : SPT_SCHEDULE_SPLIT;
    c->last_specialized = false;
    c->last_ranges = false;
    while (done < n_frames) {
        const uint32_t f = std::min(c->frames_per_pass, n_frames - done);
        p.first_frame = first_frame + done;
        p.n_frames = f;
        p.n_paths = f * c->pixels;
        EventPair ev;
        if (c->cfg.max_bounces == 0) {  // no segment traced: every path's radiance is 0
            SPT_HIP(c, hipMemsetAsync(c->radiance, 0, sizeof(float4) * (size_t)p.n_paths, on_stream(c)));
            SPT_HIP(c, hipMemsetAsync(c->counts, 0, sizeof(uint32_t) * 2 * (kMaxBounces + 1) * c->n_sub, on_stream(c)));
        }
        const uint32_t wave_bounces = std::min(c->cfg.max_bounces, schedule_tail(c));
        const bool fused = schedule_fused(c);
        for (uint32_t b = 0; b < wave_bounces; ++b) {
            if (fused) {  // extend + shade in one launch (timed as "shade")
                if (c->profiling && !c->span && begin_event(c, ev, 1, b) != SPT_OK) return SPT_ERR_HIP;
                launch_bounce(p, b, on_stream(c));
                if (c->profiling && !c->span && end_event(c, ev) != SPT_OK) return SPT_ERR_HIP;
                continue;
            }
            if (c->profiling && !c->span && begin_event(c, ev, 0, b) != SPT_OK) return SPT_ERR_HIP;
            if ((c->cfg.flags & SPT_FLAG_SORTED_RAYS) && b > 0 && c->n_nodes && c->ray_perm)
                launch_extend_sorted(p, b, on_stream(c));  // the binning is timed with the extend it serves
            else
                launch_extend(p, b, on_stream(c));
            if (c->profiling && !c->span && end_event(c, ev) != SPT_OK) return SPT_ERR_HIP;
            if (c->profiling && !c->span && begin_event(c, ev, 1, b) != SPT_OK) return SPT_ERR_HIP;
            launch_shade(p, b, on_stream(c));
            if (c->profiling && !c->span && end_event(c, ev) != SPT_OK) return SPT_ERR_HIP;
        }
        if (wave_bounces < c->cfg.max_bounces) {  // thinned queues: finish every path in one launch
            if (c->profiling && !c->span && begin_event(c, ev, 3, wave_bounces) != SPT_OK) return SPT_ERR_HIP;
            launch_trace_tail(p, wave_bounces, on_stream(c));
            if (c->profiling && !c->span && end_event(c, ev) != SPT_OK) return SPT_ERR_HIP;
        }
        if (c->profiling && !c->span && begin_event(c, ev, 2) != SPT_OK) return SPT_ERR_HIP;
        launch_accumulate(p, on_stream(c));
        if (c->profiling && !c->span && end_event(c, ev) != SPT_OK) return SPT_ERR_HIP;
        SPT_HIP(c, hipGetLastError());
        done += f;
        c->passes++;
    }
    c->frames += n_frames;
    c->paths += (uint64_t)n_frames * c->pixels;
    c->frame_count += n_frames;
    return SPT_OK;
}

// The caller waits for the frame (spt_synchronize, the resolves)
// (polling an event recorded after the frame instead measured the same)
static hipError_t wait_frame(spt_ctx* c) { return hipStreamSynchronize(on_stream(c)); }

int spt_synchronize(spt_ctx* c) {
    if (!c) return SPT_ERR_INVALID;
    SPT_HIP(c, hipSetDevice(c->device));
    SPT_HIP(c, wait_frame(c));
    return SPT_OK;
}

int spt_shard_pixels(const spt_ctx* c, uint64_t* n) {
    if (!c || !n) return SPT_ERR_INVALID;
    if (!c->configured) return SPT_ERR_NOT_CONFIGURED;
    *n = c->pixels;
    return SPT_OK;
}

int spt_read_accum(spt_ctx* c, float* host_rgba) {
    if (!c || !host_rgba) return SPT_ERR_INVALID;
    if (!c->configured) return fail(c, SPT_ERR_NOT_CONFIGURED, "not configured");
    SPT_HIP(c, hipSetDevice(c->device));
    if (c->pixels == 0) return SPT_OK;
    SPT_HIP(c, hipMemcpyAsync(host_rgba, c->accum, sizeof(float4) * c->pixels, hipMemcpyDeviceToHost, on_stream(c)));
    SPT_HIP(c, hipStreamSynchronize(on_stream(c)));
    return SPT_OK;
}

int spt_accum_device_ptr(spt_ctx* c, void** dptr, size_t* bytes) {
    if (!c || !dptr || !bytes) return SPT_ERR_INVALID;
    if (!c->configured) return fail(c, SPT_ERR_NOT_CONFIGURED, "not configured");
    *dptr = c->accum;
    *bytes = sizeof(float4) * (size_t)c->pixels;
    c->accum_shared = true;
    return SPT_OK;
}

int spt_copy_accum_device(spt_ctx* c, void* dst) {
    if (!c || !dst) return SPT_ERR_INVALID;
    if (!c->configured) return fail(c, SPT_ERR_NOT_CONFIGURED, "not configured");
    SPT_HIP(c, hipSetDevice(c->device));
    if (c->pixels == 0) return SPT_OK;
    SPT_HIP(c, hipMemcpyAsync(dst, c->accum, sizeof(float4) * c->pixels, hipMemcpyDeviceToDevice, on_stream(c)));
    return SPT_OK;
}

int spt_resolve_rgba8(spt_ctx* c, uint32_t frame_count, uint32_t* host_out) {
    return spt_resolve_rgba8_exposure(c, frame_count, 1.0f, host_out);
}

// The ctx's image as RGBA8 in host_out, waited for; launch(out, stream) enqueues the kernel that writes it.
extern "C++" {  // (a template inside the C-ABI's linkage block)
template <class Launch>
static int resolve_image_by(spt_ctx* c, uint32_t* host_out, Launch&& launch) {
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
}  // extern "C++"

// img / divisor as RGBA8 in host_out, waited for (the sums and a frame count, or a mean and 1)
static int resolve_image(spt_ctx* c, const float4* img, float divisor, float exposure, uint32_t* host_out) {
    return resolve_image_by(c, host_out, [&](uint32_t* out, hipStream_t s) {
        launch_resolve(img, c->pixels, divisor, exposure, out, s);
    });
}

int spt_resolve_rgba8_exposure(spt_ctx* c, uint32_t frame_count, float exposure, uint32_t* host_out) {
    if (!c || !host_out) return SPT_ERR_INVALID;
    if (!c->configured) return fail(c, SPT_ERR_NOT_CONFIGURED, "not configured");
    if (frame_count == 0) return fail(c, SPT_ERR_INVALID, "No frames rendered yet");  // CPUPathTracer.cpp:89
    return resolve_image(c, c->accum, (float)frame_count, exposure, host_out);
}

int spt_render_resolve_rgba8(spt_ctx* c, uint32_t first_frame, uint32_t n_frames, uint32_t frame_count, float exposure,
                             uint32_t* host_out) {
    if (!c || !host_out) return SPT_ERR_INVALID;
    if (frame_count == 0) return fail(c, SPT_ERR_INVALID, "No frames rendered yet");  // CPUPathTracer.cpp:89
    // fused only into the registered buffer (device-mapped host memory) and only by a k_frame launch;
    // any other call renders, then resolves as spt_resolve_rgba8_exposure does (same pixels)
    // (not while spt_set_profiling counts segments: the fused kernels carry no counters)
    const bool fuse = c->configured && !c->counters && host_out == c->out_host &&
                      sizeof(uint32_t) * (size_t)c->pixels <= c->out_bytes;
    c->fuse_frames = fuse ? (float)frame_count : 0.0f;
    c->fuse_exposure = exposure;
    c->fused = false;
    const int rc = spt_render(c, first_frame, n_frames);
    const bool fused = c->fused;
    c->fuse_frames = 0.0f;
    c->fused = false;
    if (rc != SPT_OK) return rc;
    if (!fused) return spt_resolve_rgba8_exposure(c, frame_count, exposure, host_out);
    SPT_HIP(c, wait_frame(c));  // (the frame's stores have reached host memory)
    return SPT_OK;
}

int spt_register_host_output(spt_ctx* c, void* host_out, size_t bytes) {
    if (!c) return SPT_ERR_INVALID;
    if ((host_out == nullptr) != (bytes == 0)) return fail(c, SPT_ERR_INVALID, "host output: pointer and size disagree");
    SPT_HIP(c, hipSetDevice(c->device));
    if (c->out_host) {
        SPT_HIP(c, hipStreamSynchronize(on_stream(c)));  // no resolve may still be writing it
        const hipError_t e = hipHostUnregister(c->out_host);
        c->out_host = c->out_dev = nullptr;
        c->out_bytes = 0;
        if (e != hipSuccess) return fail(c, SPT_ERR_HIP, std::string("hipHostUnregister: ") + hipGetErrorString(e));
    }
    if (!host_out) return SPT_OK;
    SPT_HIP(c, hipHostRegister(host_out, bytes, hipHostRegisterMapped));
    void* dev = nullptr;
    const hipError_t e = hipHostGetDevicePointer(&dev, host_out, 0);
    if (e != hipSuccess) {
        (void)hipHostUnregister(host_out);
        return fail(c, SPT_ERR_HIP, std::string("hipHostGetDevicePointer: ") + hipGetErrorString(e));
    }
    c->out_host = host_out;
    c->out_dev = dev;
    c->out_bytes = bytes;
    return SPT_OK;
}

int spt_assemble_rows(spt_ctx* c, const void* gathered, void* out) {
    if (!c || !gathered || !out) return SPT_ERR_INVALID;
    if (!c->configured) return fail(c, SPT_ERR_NOT_CONFIGURED, "not configured");
    SPT_HIP(c, hipSetDevice(c->device));
    const uint32_t world = c->cfg.shard_count;
    const uint32_t rows_max = (c->cfg.height + world - 1) / world;
    launch_assemble_rows((const float4*)gathered, (float4*)out, c->cfg.width, c->cfg.height, world, rows_max, on_stream(c));
    SPT_HIP(c, hipGetLastError());
    return SPT_OK;
}

int spt_set_env_map(spt_ctx* c, const float* rgba, uint32_t width, uint32_t height) {
    if (!c) return SPT_ERR_INVALID;
    if (rgba && (width == 0 || height == 0 || (uint64_t)width * height >= (1ull << 28)))
        return fail(c, SPT_ERR_INVALID, "environment map: bad size");
    SPT_HIP(c, hipSetDevice(c->device));
    SPT_HIP(c, hipStreamSynchronize(on_stream(c)));
    c->d_env.reset();
    c->env_w = c->env_h = 0;
    if (rgba) {
        const size_t texels = (size_t)width * height;
        if (!c->d_env.alloc(texels)) return fail(c, SPT_ERR_HIP, "spt_set_env_map: allocation failed");
        SPT_HIP(c, hipMemcpy(c->d_env, rgba, sizeof(float4) * texels, hipMemcpyHostToDevice));
        c->env_w = width;
        c->env_h = height;
    }
    c->derived.drop(Change::Sky);
    if (c->configured) return spt_reset(c);  // a different sky: the accumulation restarts
    return SPT_OK;
}

// nullptr: valid
static const char* camera_error(const spt_camera& cam) {
    double w2 = 0.0;
    for (int a = 0; a < 3; ++a) {
        if (!std::isfinite(cam.origin[a]) || !std::isfinite(cam.u[a]) || !std::isfinite(cam.v[a]) ||
            !std::isfinite(cam.w[a]))
            return "camera: non-finite value";
        w2 += (double)cam.w[a] * cam.w[a];
    }
    if (!(w2 > 0.0)) return "camera: w (forward) is zero";
    if (cam.flags & ~(uint32_t)SPT_CAMERA_JITTER) return "camera: unknown flags";
    if (cam.reserved[0] | cam.reserved[1] | cam.reserved[2]) return "camera: reserved must be 0";
    return nullptr;
}

// A BVH scene's boxes are padded for ray origins inside max(scene magnitude, reach) (scene.h). A camera
// outside the scene's magnitude, or one that comes back into it, changes that: the tree is refitted with
// the new padding and uploaded again (spt_update_prims' path with no edit: the node array, the stacks if the
// collapse deepens; the caller drops what a camera change drops). A camera that stays inside the scene's
// magnitude changes nothing and uploads nothing.
static int repad_for_camera(spt_ctx* c) {
    if (!c->has_scene || c->h_nodes.empty()) return SPT_OK;
    if (std::max(c->scene_mag, camera_reach(c)) == std::max(c->scene_mag, c->pad_reach)) return SPT_OK;
    return refit_scene(c, nullptr, nullptr, 0, false);
}

int spt_set_camera(spt_ctx* c, const spt_camera* cam) {
    if (!c) return SPT_ERR_INVALID;
    if (cam) {
        if (const char* msg = camera_error(*cam)) return fail(c, SPT_ERR_INVALID, msg);
        // the device record; a lens stays, on the new camera's u and v
        const spt_camera old = c->camera;
        c->camera = *cam;
        if (const int rc = write_camera_record(c); rc != SPT_OK) {
            c->camera = old;
            return rc;
        }
    } else {
        c->has_lens = false;  // (the reference's pinhole has no lens)
    }
    c->has_camera = cam != nullptr;
    c->derived.drop(Change::Camera);
    if (const int rc = repad_for_camera(c); rc != SPT_OK) return rc;
    prefetch_flat(c);  // (a flat scene's kernels are compiled for having a camera or none, too)
    if (c->configured) return spt_reset(c);  // another view: the accumulation restarts
    return SPT_OK;
}

// nullptr: valid
static const char* lens_error(const spt_lens& l) {
    if (!std::isfinite(l.radius) || l.radius < 0.0f) return "lens: radius must be finite and >= 0";
    if (!std::isfinite(l.focus_distance) || !(l.focus_distance > 0.0f)) return "lens: focus_distance must be finite and > 0";
    if (l.reserved[0] | l.reserved[1]) return "lens: reserved must be 0";
    return nullptr;
}

int spt_set_camera_lens(spt_ctx* c, const spt_lens* lens) {
    if (!c) return SPT_ERR_INVALID;
    if (!c->has_camera) return fail(c, SPT_ERR_INVALID, "spt_set_camera_lens without a camera (spt_set_camera)");
    if (lens)
        if (const char* msg = lens_error(*lens)) return fail(c, SPT_ERR_INVALID, msg);
    const bool had = c->has_lens;
    const spt_lens old = c->lens;
    c->has_lens = lens != nullptr && lens->radius != 0.0f;  // (radius 0: the pinhole, and its kernels)
    if (c->has_lens) c->lens = *lens;
    if (const int rc = write_camera_record(c); rc != SPT_OK) {
        c->has_lens = had;
        c->lens = old;
        return rc;
    }
    c->derived.drop(Change::Lens);
    if (const int rc = repad_for_camera(c); rc != SPT_OK) return rc;
    prefetch_flat(c);
    if (c->configured) return spt_reset(c);
    return SPT_OK;
}

int spt_set_material_models(spt_ctx* c, const spt_material_model* models, uint32_t n) {
    if (!c) return SPT_ERR_INVALID;
    if (!c->has_scene) return fail(c, SPT_ERR_NO_SCENE, "spt_set_material_models before spt_set_scene");
    if (models) {
        if (n != (uint32_t)c->h_mats.size())
            return fail(c, SPT_ERR_INVALID, "spt_set_material_models: n is not the scene's material count");
        for (uint32_t i = 0; i < n; ++i)
            if (const char* msg = model_error(models[i])) return fail(c, SPT_ERR_INVALID, msg);
    }
    SPT_HIP(c, hipSetDevice(c->device));
    SPT_HIP(c, hipStreamSynchronize(on_stream(c)));  // (a launch in flight reads the old words)
    const std::vector<spt_material_model> old = c->h_models;
    if (models) c->h_models.assign(models, models + n);
    else c->h_models.clear();
    if (upload_materials(c) != SPT_OK) {
        c->h_models = old;
        return SPT_ERR_HIP;
    }
    c->derived.drop(Change::Materials);
    if (c->configured) return spt_reset(c);  // other materials: the accumulation restarts
    return SPT_OK;
}

int spt_bsdf_sample(const spt_material_model* model, const float d[3], const float n[3], int entering, uint32_t flags,
                    uint32_t* rng, float dir_out[3], int* transmitted, int* absorbed) {
    if (!model || !d || !n || !rng || !dir_out || !transmitted || !absorbed) return SPT_ERR_INVALID;
    if (model_error(*model)) return SPT_ERR_INVALID;
    const F3 dv{d[0], d[1], d[2]}, nv{n[0], n[1], n[2]};
    uint32_t state = *rng;
    Scatter s{F3{0.f, 0.f, 0.f}, false, false};
    if (model->kind == SPT_MAT_DIFFUSE) {
        s.dir = bounce_dir(nv, state, flags);
    } else {
        const F3 nf = entering ? nv : F3{-nv.x, -nv.y, -nv.z};
        s = bsdf_scatter(model->kind, model->param, dv, nf, entering != 0, flags, state);
    }
    *rng = state;
    dir_out[0] = s.dir.x;
    dir_out[1] = s.dir.y;
    dir_out[2] = s.dir.z;
    *transmitted = s.transmitted ? 1 : 0;
    *absorbed = s.absorbed ? 1 : 0;
    return SPT_OK;
}

// ---- first-hit features and the denoiser ---------------------------------------------------------

namespace {
const spt_denoise_params kDenoiseDefaults = {5u, 1.0f, 0.05f, 5u, {0u, 0u, 0u, 0u}};
// nullptr: valid
const char* denoise_params_error(const spt_denoise_params& p) {
    if (p.levels < 1u || p.levels > kAtrousMaxLevels) return "spt_denoise_params: levels outside 1..6";
    if (!(p.sigma_color > 0.0f) || !std::isfinite(p.sigma_color)) return "spt_denoise_params: sigma_color must be > 0 and finite";
    if (!(p.sigma_plane > 0.0f) || !std::isfinite(p.sigma_plane)) return "spt_denoise_params: sigma_plane must be > 0 and finite";
    if (p.normal_power_log2 > kAtrousMaxNormalPower) return "spt_denoise_params: normal_power_log2 outside 0..7";
    if (p.reserved[0] | p.reserved[1] | p.reserved[2] | p.reserved[3]) return "spt_denoise_params: reserved must be 0";
    return nullptr;
}
// the images are those of the current scene, camera and configuration (rendered now if they are not)
int ensure_features(spt_ctx* c) {
    if (!c->has_scene) return fail(c, SPT_ERR_NO_SCENE, "Scene not set before rendering");
    if (!c->configured) return fail(c, SPT_ERR_NOT_CONFIGURED, "features before spt_configure");
    SPT_HIP(c, hipSetDevice(c->device));
    if (c->derived.valid(kFeatures) || c->pixels == 0) return SPT_OK;
    for (Dev<float4>* img : {&c->feat_a, &c->feat_b, &c->feat_albedo})
        if (const int rc = ensure_buf(c, *img, c->pixels, "spt_render_features"); rc != SPT_OK) return rc;
    launch_features(base_params(c), c->d_mat_map, c->feat_a, c->feat_b, c->feat_albedo, on_stream(c));
    SPT_HIP(c, hipGetLastError());
    c->derived.produced(kFeatures);
    return SPT_OK;
}
}  // namespace

int spt_render_features(spt_ctx* c) {
    if (!c) return SPT_ERR_INVALID;
    return ensure_features(c);
}

int spt_read_features(spt_ctx* c, float* feat_a, float* feat_b, float* albedo) {
    if (!c) return SPT_ERR_INVALID;
    const int rc = ensure_features(c);
    if (rc != SPT_OK || c->pixels == 0) return rc;
    const size_t bytes = sizeof(float4) * c->pixels;
    if (feat_a) SPT_HIP(c, hipMemcpyAsync(feat_a, c->feat_a, bytes, hipMemcpyDeviceToHost, on_stream(c)));
    if (feat_b) SPT_HIP(c, hipMemcpyAsync(feat_b, c->feat_b, bytes, hipMemcpyDeviceToHost, on_stream(c)));
    if (albedo) SPT_HIP(c, hipMemcpyAsync(albedo, c->feat_albedo, bytes, hipMemcpyDeviceToHost, on_stream(c)));
    SPT_HIP(c, hipStreamSynchronize(on_stream(c)));
    return SPT_OK;
}

int spt_features_device_ptr(spt_ctx* c, void** feat_a, void** feat_b, void** albedo, size_t* bytes) {
    if (!c || !bytes) return SPT_ERR_INVALID;
    const int rc = ensure_features(c);
    if (rc != SPT_OK) return rc;
    if (feat_a) *feat_a = c->feat_a;
    if (feat_b) *feat_b = c->feat_b;
    if (albedo) *albedo = c->feat_albedo;
    *bytes = sizeof(float4) * (size_t)c->pixels;
    return SPT_OK;
}

int spt_denoise_params_default(spt_denoise_params* out) {
    if (!out) return SPT_ERR_INVALID;
    *out = kDenoiseDefaults;
    return SPT_OK;
}

// the filter over `in` / divisor (divisor 0: `in` is already the mean), into the ctx's denoised image
static int denoise_image(spt_ctx* c, const float4* in0, float divisor, const spt_denoise_params* params) {
    if (!c->has_scene) return fail(c, SPT_ERR_NO_SCENE, "Scene not set before rendering");
    if (!c->configured) return fail(c, SPT_ERR_NOT_CONFIGURED, "spt_denoise before spt_configure");
    const spt_denoise_params p = params ? *params : kDenoiseDefaults;
    if (const char* msg = denoise_params_error(p)) return fail(c, SPT_ERR_INVALID, msg);
    if (c->cfg.shard_count != 1u) return fail(c, SPT_ERR_INVALID, "spt_denoise needs the whole image (shard_count 1)");
    // (the straight form's grid has a block row per 4 image rows)
    if (c->cfg.height > 4u * 65535u) return fail(c, SPT_ERR_INVALID, "spt_denoise: image taller than 262140 rows");
    const int rc = ensure_features(c);
    if (rc != SPT_OK || c->pixels == 0) return rc;
    for (Dev<float4>& img : c->dn)
        if (const int rc = ensure_buf(c, img, c->pixels, "spt_denoise"); rc != SPT_OK) return rc;
    c->derived.begin(kDenoised);
    c->dn_guided = false;
    const int forced = c->dn_form;  // spt_set_denoise_form: one form for every level (measurement), or -1
    for (uint32_t l = 0; l < p.levels; ++l) {
        const AtrousLevel lv = atrous_level(l, p.sigma_color, p.sigma_plane, p.normal_power_log2);
        const float4* in = l == 0 ? in0 : c->dn[(l - 1u) & 1u];
        launch_atrous(forced >= 0 ? forced : atrous_form_of_step(lv.step), in, l == 0 ? divisor : 0.0f,
                      c->feat_a, c->feat_b, c->dn[l & 1u], c->cfg.width, c->cfg.height, lv, on_stream(c));
        SPT_HIP(c, hipGetLastError());
    }
    c->derived.produced_denoised((int)((p.levels - 1u) & 1u));
    return SPT_OK;
}

int spt_denoise(spt_ctx* c, uint32_t frame_count, const spt_denoise_params* params) {
    if (!c) return SPT_ERR_INVALID;
    // (no scene or configuration is reported first, by denoise_image; a divisor of 0 would mean "already a mean")
    if (c->has_scene && c->configured && frame_count == 0) return fail(c, SPT_ERR_INVALID, "No frames rendered yet");
    return denoise_image(c, c->accum, (float)frame_count, params);
}

int spt_denoise_guided(spt_ctx* c, uint32_t frame_count, const spt_guided_params* params) {
    if (!c) return SPT_ERR_INVALID;
    if (!c->has_scene) return fail(c, SPT_ERR_NO_SCENE, "Scene not set before rendering");
    if (!c->configured) return fail(c, SPT_ERR_NOT_CONFIGURED, "spt_denoise_guided before spt_configure");
    if (frame_count == 0) return fail(c, SPT_ERR_INVALID, "No frames rendered yet");
    const spt_guided_params p = params ? *params : kGuidedDefaults;
    if (const char* msg = guided_params_error(p)) return fail(c, SPT_ERR_INVALID, msg);
    if (c->cfg.shard_count != 1u) return fail(c, SPT_ERR_INVALID, "spt_denoise_guided needs the whole image (shard_count 1)");
    if (c->cfg.height > 4u * 65535u) return fail(c, SPT_ERR_INVALID, "spt_denoise_guided: image taller than 262140 rows");
    if (c->noise_batches < 2 || !c->noise_state)
        return fail(c, SPT_ERR_INVALID, "spt_denoise_guided: fewer than two spt_noise_update batches since the accumulation restarted");
    const int rc = ensure_features(c);
    if (rc != SPT_OK || c->pixels == 0) return rc;
    for (Dev<float4>& img : c->dn)
        if (const int rc = ensure_buf(c, img, c->pixels, "spt_denoise_guided"); rc != SPT_OK) return rc;
    for (Dev<float>& plane : c->dn_var)
        if (const int rc = ensure_buf(c, plane, c->pixels, "spt_denoise_guided"); rc != SPT_OK) return rc;
    c->derived.begin(kDenoised);
    c->dn_guided = false;
    // the variance plane "the level before the first" wrote: slot 1, so that level l reads slot (l - 1) & 1
    launch_guided_variance(c->noise_state, c->dn_var[1], c->cfg.width, c->cfg.height, guided_inv(c->noise_batches, frame_count),
                           p.prefilter != 0u, on_stream(c));
    SPT_HIP(c, hipGetLastError());
    const int forced = c->dn_form;  // spt_set_denoise_form: one form for every level (measurement), or -1
    for (uint32_t l = 0; l < p.levels; ++l) {
        const GuidedLevel lv = guided_level(l, p);
        const float4* in = l == 0 ? (const float4*)c->accum : (const float4*)c->dn[(l - 1u) & 1u];
        launch_guided_level(forced >= 0 ? forced : guided_form_of_step(lv.step), in, l == 0 ? (float)frame_count : 0.0f,
                            c->dn_var[(l + 1u) & 1u], c->feat_a, c->feat_b, c->dn[l & 1u], c->dn_var[l & 1u],
                            c->cfg.width, c->cfg.height, lv, on_stream(c));
        SPT_HIP(c, hipGetLastError());
    }
    c->derived.produced_denoised((int)((p.levels - 1u) & 1u));
    c->dn_guided = true;
    return SPT_OK;
}

int spt_read_denoised_variance(spt_ctx* c, float* host_v) {
    if (!c || !host_v) return SPT_ERR_INVALID;
    if (!c->derived.valid(kDenoised) || !c->dn_guided)
        return fail(c, SPT_ERR_INVALID, "no guided denoised image: spt_denoise_guided first");
    SPT_HIP(c, hipSetDevice(c->device));
    SPT_HIP(c, hipMemcpyAsync(host_v, c->dn_var[c->derived.dn_result], sizeof(float) * c->pixels, hipMemcpyDeviceToHost, on_stream(c)));
    SPT_HIP(c, hipStreamSynchronize(on_stream(c)));
    return SPT_OK;
}

int spt_set_denoise_form(spt_ctx* c, int form) {
    if (!c) return SPT_ERR_INVALID;
    if (form != -1 && form != kAtrousStraight && form != kAtrousTiled)
        return fail(c, SPT_ERR_INVALID, "spt_set_denoise_form: -1 (automatic), 0 (straight) or 1 (tiled)");
    c->dn_form = form;
    return SPT_OK;
}

// ---- the post-processed images: denoised, active history, blended ---------------------------------
// Each is described once: a pointer, whether it is valid (spt_ctx_state.h) and what to say when it is not.
// Reading one back, handing out its address and resolving it to RGBA8 are one body each, for all of them.
enum PostImage { kImgDenoised, kImgHistory, kImgBlended };
// the image, or nullptr with the ctx's error set: there is none
static float4* post_image(spt_ctx* c, PostImage which) {
    const DerivedState& d = c->derived;
    const struct {
        float4* img;  // (a valid one was allocated: never nullptr)
        const char* missing;
    } images[] = {{d.valid(kDenoised) ? c->dn[d.dn_result] : nullptr, "no denoised image: spt_denoise first"},
                  {d.valid(kHistory) ? c->hist : nullptr, "no active history: spt_reproject first"},
                  {d.valid(kBlended) ? c->blend : nullptr, "no blended image: spt_history_blend first"}};
    if (!images[which].img) fail(c, SPT_ERR_INVALID, images[which].missing);
    return images[which].img;
}

static int read_image(spt_ctx* c, PostImage which, float* host_rgba) {
    if (!c || !host_rgba) return SPT_ERR_INVALID;
    const float4* img = post_image(c, which);
    if (!img) return SPT_ERR_INVALID;
    SPT_HIP(c, hipSetDevice(c->device));
    SPT_HIP(c, hipMemcpyAsync(host_rgba, img, sizeof(float4) * c->pixels, hipMemcpyDeviceToHost, on_stream(c)));
    SPT_HIP(c, hipStreamSynchronize(on_stream(c)));
    return SPT_OK;
}

static int image_device_ptr(spt_ctx* c, PostImage which, void** dptr, size_t* bytes) {
    if (!c || !dptr || !bytes) return SPT_ERR_INVALID;
    float4* img = post_image(c, which);
    if (!img) return SPT_ERR_INVALID;
    *dptr = img;
    *bytes = sizeof(float4) * (size_t)c->pixels;
    return SPT_OK;
}

// spt_resolve_rgba8_exposure of an image that is already a mean (divisor 1)
static int resolve_mean_rgba8(spt_ctx* c, PostImage which, float exposure, uint32_t* host_out) {
    if (!c || !host_out) return SPT_ERR_INVALID;
    const float4* img = post_image(c, which);
    return img ? resolve_image(c, img, 1.0f, exposure, host_out) : SPT_ERR_INVALID;
}

int spt_read_denoised(spt_ctx* c, float* host_rgba) { return read_image(c, kImgDenoised, host_rgba); }
int spt_denoised_device_ptr(spt_ctx* c, void** dptr, size_t* bytes) { return image_device_ptr(c, kImgDenoised, dptr, bytes); }
int spt_resolve_denoised_rgba8(spt_ctx* c, float exposure, uint32_t* host_out) {
    return resolve_mean_rgba8(c, kImgDenoised, exposure, host_out);
}

int spt_atrous_host(const float* rgba, const float* feat_a, const float* feat_b, uint32_t width, uint32_t height,
                    const spt_denoise_params* params, float* out) {
    if (!rgba || !feat_a || !feat_b || !out || width == 0 || height == 0) return SPT_ERR_INVALID;
    if ((uint64_t)width * height >= (1ull << 31)) return SPT_ERR_INVALID;
    const spt_denoise_params p = params ? *params : kDenoiseDefaults;
    if (denoise_params_error(p)) return SPT_ERR_INVALID;
    const size_t n = (size_t)width * height;
    const int w = (int)width, h = (int)height;
    auto px = [](const float* a, size_t i) { return make_float4(a[4 * i], a[4 * i + 1], a[4 * i + 2], a[4 * i + 3]); };
    std::vector<float> buf[2] = {std::vector<float>(4 * n), std::vector<float>(4 * n)};
    const float* in = rgba;
    for (uint32_t l = 0; l < p.levels; ++l) {
        const AtrousLevel lv = atrous_level(l, p.sigma_color, p.sigma_plane, p.normal_power_log2);
        float* dst = buf[l & 1u].data();
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < w; ++x) {
                const size_t at = (size_t)y * width + (size_t)x;
                const float4 cp = px(in, at);
                const float4 o = atrous_pixel(atrous_tap(cp, px(feat_a, at), px(feat_b, at)), cp.w, x, y, w, h, lv,
                                              [&](int, int, int qx, int qy) {
                                                  const size_t q = (size_t)qy * width + (size_t)qx;
                                                  return atrous_tap(px(in, q), px(feat_a, q), px(feat_b, q));
                                              });
                dst[4 * at + 0] = o.x;
                dst[4 * at + 1] = o.y;
                dst[4 * at + 2] = o.z;
                dst[4 * at + 3] = o.w;
            }
        in = dst;
    }
    std::memcpy(out, in, sizeof(float) * 4 * n);
    return SPT_OK;
}

// ---- temporal reprojection ------------------------------------------------------------------------

namespace {
const spt_reproject_params kReprojectDefaults = {32.0f, 0.9f, 0.01f, 0.01f, {0u, 0u, 0u, 0u}};
// nullptr: valid
const char* reproject_params_error(const spt_reproject_params& p) {
    if (!std::isfinite(p.max_history) || !(p.max_history >= 1.0f)) return "spt_reproject_params: max_history must be finite and >= 1";
    if (!std::isfinite(p.normal_min)) return "spt_reproject_params: normal_min must be finite";
    if (!std::isfinite(p.plane_tolerance) || !(p.plane_tolerance >= 0.0f)) return "spt_reproject_params: plane_tolerance must be finite and >= 0";
    if (!std::isfinite(p.min_weight) || !(p.min_weight > 0.0f)) return "spt_reproject_params: min_weight must be finite and > 0";
    if (p.reserved[0] | p.reserved[1] | p.reserved[2] | p.reserved[3]) return "spt_reproject_params: reserved must be 0";
    return nullptr;
}
// what spt_history_capture, spt_reproject and spt_history_blend share: a whole image, and for the first two
// (features) its current feature images
int history_ready(spt_ctx* c, const char* who, bool features) {
    if (!c->has_scene) return fail(c, SPT_ERR_NO_SCENE, "Scene not set before rendering");
    if (!c->configured) return fail(c, SPT_ERR_NOT_CONFIGURED, std::string(who) + " before spt_configure");
    if (c->cfg.shard_count != 1u) return fail(c, SPT_ERR_INVALID, std::string(who) + " needs the whole image (shard_count 1)");
    // (k_reproject's grid has a block row per 4 image rows)
    if (c->cfg.height > 4u * 65535u) return fail(c, SPT_ERR_INVALID, std::string(who) + ": image taller than 262140 rows");
    if (features) return ensure_features(c);
    SPT_HIP(c, hipSetDevice(c->device));
    return SPT_OK;
}
}  // namespace

int spt_reproject_params_default(spt_reproject_params* out) {
    if (!out) return SPT_ERR_INVALID;
    *out = kReprojectDefaults;
    return SPT_OK;
}

int spt_history_capture(spt_ctx* c, uint32_t frame_count) {
    if (!c) return SPT_ERR_INVALID;
    if (const int rc = history_ready(c, "spt_history_capture", true); rc != SPT_OK) return rc;
    if (frame_count == 0) return fail(c, SPT_ERR_INVALID, "No frames rendered yet");
    if (const int rc = ensure_buf(c, c->hist_view, 3 * (size_t)c->pixels, "spt_history_capture"); rc != SPT_OK) return rc;
    c->derived.begin(kCapturedView);
    const int layout = c->hist_layout >= 0 ? c->hist_layout : kHistoryDefault;
    launch_history_capture(layout, c->accum, (float)frame_count, c->derived.valid(kHistory) ? c->hist : nullptr, c->feat_a, c->feat_b,
                           c->hist_view, c->pixels, on_stream(c));
    SPT_HIP(c, hipGetLastError());
    c->hist_view_layout = layout;
    c->hist_view_has_camera = c->has_camera;
    c->hist_view_camera = c->camera;
    c->derived.produced(kCapturedView);
    return SPT_OK;
}

int spt_reproject(spt_ctx* c, const spt_reproject_params* params) {
    if (!c) return SPT_ERR_INVALID;
    const spt_reproject_params p = params ? *params : kReprojectDefaults;
    if (const char* msg = reproject_params_error(p)) return fail(c, SPT_ERR_INVALID, msg);
    if (const int rc = history_ready(c, "spt_reproject", true); rc != SPT_OK) return rc;
    if (!c->derived.valid(kCapturedView)) return fail(c, SPT_ERR_INVALID, "no captured view: spt_history_capture first");
    if (const int rc = ensure_buf(c, c->hist, c->pixels, "spt_reproject"); rc != SPT_OK) return rc;
    c->derived.begin(kHistory);
    const uint32_t n_mats = (uint32_t)c->h_mats.size();
    if (c->bsdf && !c->derived.valid(kReusable)) {
        // (spt_set_material_models drained the stream before it changed the models: nothing reads the old words)
        std::vector<uint32_t> words(n_mats);
        for (uint32_t m = 0; m < n_mats; ++m) words[m] = c->h_models[m].kind == SPT_MAT_DIFFUSE ? 1u : 0u;
        if (const int rc = ensure_buf(c, c->d_reusable, n_mats, "spt_reproject"); rc != SPT_OK) return rc;
        SPT_HIP(c, hipMemcpy(c->d_reusable, words.data(), sizeof(uint32_t) * n_mats, hipMemcpyHostToDevice));
        c->derived.produced(kReusable);
    }
    const ReprojectView v = reproject_view(c->hist_view_has_camera ? &c->hist_view_camera : nullptr);
    launch_reproject(c->hist_view_layout, c->feat_a, c->feat_b, c->hist_view, c->hist, c->cfg.width, c->cfg.height, v, p,
                     c->bsdf ? c->d_reusable : nullptr, n_mats, on_stream(c));
    SPT_HIP(c, hipGetLastError());
    c->derived.produced(kHistory);
    return SPT_OK;
}

int spt_history_clear(spt_ctx* c) {
    if (!c) return SPT_ERR_INVALID;
    c->derived.drop(Change::HistoryClear);
    return SPT_OK;
}

int spt_read_history(spt_ctx* c, float* host_rgba) { return read_image(c, kImgHistory, host_rgba); }
int spt_history_device_ptr(spt_ctx* c, void** dptr, size_t* bytes) { return image_device_ptr(c, kImgHistory, dptr, bytes); }

int spt_history_blend(spt_ctx* c, uint32_t frame_count) {
    if (!c) return SPT_ERR_INVALID;
    if (const int rc = history_ready(c, "spt_history_blend", false); rc != SPT_OK) return rc;
    if (frame_count == 0) return fail(c, SPT_ERR_INVALID, "No frames rendered yet");
    if (const int rc = ensure_buf(c, c->blend, c->pixels, "spt_history_blend"); rc != SPT_OK) return rc;
    c->derived.begin(kBlended);
    launch_history_blend(c->accum, (float)frame_count, c->derived.valid(kHistory) ? c->hist : nullptr, c->blend, c->pixels, on_stream(c));
    SPT_HIP(c, hipGetLastError());
    c->derived.produced(kBlended);
    return SPT_OK;
}

int spt_read_blended(spt_ctx* c, float* host_rgba) { return read_image(c, kImgBlended, host_rgba); }
int spt_blended_device_ptr(spt_ctx* c, void** dptr, size_t* bytes) { return image_device_ptr(c, kImgBlended, dptr, bytes); }
int spt_resolve_blended_rgba8(spt_ctx* c, float exposure, uint32_t* host_out) {
    return resolve_mean_rgba8(c, kImgBlended, exposure, host_out);
}

int spt_denoise_blended(spt_ctx* c, const spt_denoise_params* params) {
    if (!c) return SPT_ERR_INVALID;
    const float4* img = post_image(c, kImgBlended);
    return img ? denoise_image(c, img, 0.0f, params) : SPT_ERR_INVALID;
}

int spt_set_history_layout(spt_ctx* c, int layout) {
    if (!c) return SPT_ERR_INVALID;
    if (layout != -1 && layout != kHistoryPlanes && layout != kHistoryRecords)
        return fail(c, SPT_ERR_INVALID, "spt_set_history_layout: -1 (automatic), 0 (three images) or 1 (48-byte records)");
    c->hist_layout = layout;
    return SPT_OK;
}

int spt_reproject_basis(const spt_camera* cam, float rows[9], float origin[3], float* j) {
    if (!rows || !origin || !j) return SPT_ERR_INVALID;
    if (cam && camera_error(*cam)) return SPT_ERR_INVALID;
    const ReprojectView v = reproject_view(cam);
    for (int a = 0; a < 3; ++a) {
        rows[a] = v.ru[a];
        rows[3 + a] = v.rv[a];
        rows[6 + a] = v.rw[a];
        origin[a] = v.o[a];
    }
    *j = v.j;
    return SPT_OK;
}

int spt_reproject_host(const spt_reproject_params* params, const spt_camera* prev_camera, uint32_t width, uint32_t height,
                       const float* cur_a, const float* cur_b, const float* hist_rgba, const float* hist_a,
                       const float* hist_b, const uint32_t* material_reusable, uint32_t n_materials, float* out) {
    if (!cur_a || !cur_b || !hist_rgba || !hist_a || !hist_b || !out || width == 0 || height == 0) return SPT_ERR_INVALID;
    if ((uint64_t)width * height >= (1ull << 31)) return SPT_ERR_INVALID;
    const spt_reproject_params p = params ? *params : kReprojectDefaults;
    if (reproject_params_error(p)) return SPT_ERR_INVALID;
    if (prev_camera && camera_error(*prev_camera)) return SPT_ERR_INVALID;
    const ReprojectView v = reproject_view(prev_camera);
    auto px = [](const float* a, size_t i) { return make_float4(a[4 * i], a[4 * i + 1], a[4 * i + 2], a[4 * i + 3]); };
    const size_t n = (size_t)width * height;
    for (size_t at = 0; at < n; ++at) {
        const float4 o = reproject_pixel(
            px(cur_a, at), px(cur_b, at), (int)width, (int)height, v, p, material_reusable, n_materials,
            [&](size_t q) { return px(hist_a, q); }, [&](size_t q) { return px(hist_b, q); },
            [&](size_t q) { return px(hist_rgba, q); });
        out[4 * at + 0] = o.x;
        out[4 * at + 1] = o.y;
        out[4 * at + 2] = o.z;
        out[4 * at + 3] = o.w;
    }
    return SPT_OK;
}

// ---- exposure and tone mapping: the luminance meter and the display resolve -------------------------

namespace {
const spt_exposure_params kExposureDefaults = {0.18f, 0.1f, 0.02f, 0.015625f, 64.0f, {0u, 0u, 0u}};
bool exposure_params_ok(const spt_exposure_params& p) {
    for (const float v : {p.target_luminance, p.low_fraction, p.high_fraction, p.min_exposure, p.max_exposure})
        if (!std::isfinite(v)) return false;
    if (!(p.target_luminance > 0.0f) || !(p.min_exposure > 0.0f) || !(p.max_exposure > 0.0f)) return false;
    if (p.min_exposure > p.max_exposure) return false;
    if (p.low_fraction < 0.0f || p.high_fraction < 0.0f) return false;
    if ((double)p.low_fraction + (double)p.high_fraction >= 1.0) return false;
    return !(p.reserved[0] | p.reserved[1] | p.reserved[2]);
}
// nullptr: valid
const char* display_error(const spt_display& d) {
    if (d.tonemap > SPT_TONEMAP_ACES) return "spt_display: unknown tonemap operator";
    if (!std::isfinite(d.exposure) || d.exposure < 0.0f) return "spt_display: exposure must be finite and >= 0";
    if (d.reserved[0] | d.reserved[1]) return "spt_display: reserved must be 0";
    return nullptr;
}
bool divisor_ok(float divisor) { return std::isfinite(divisor) && divisor > 0.0f; }

// The ctx image `image` with its divisor (the frame count for the sums, 1 for a mean), or nullptr with the
// status to return in *rc.
const float4* display_source(spt_ctx* c, uint32_t image, uint32_t frame_count, float* divisor, int* rc) {
    *rc = SPT_ERR_INVALID;
    if (image > SPT_IMAGE_BLENDED) {
        fail(c, SPT_ERR_INVALID, "unknown image: SPT_IMAGE_ACCUM, SPT_IMAGE_DENOISED or SPT_IMAGE_BLENDED");
        return nullptr;
    }
    if (!c->configured) {
        *rc = fail(c, SPT_ERR_NOT_CONFIGURED, "not configured");
        return nullptr;
    }
    *divisor = 1.0f;
    if (image != SPT_IMAGE_ACCUM) return post_image(c, image == SPT_IMAGE_DENOISED ? kImgDenoised : kImgBlended);
    if (frame_count == 0) {
        fail(c, SPT_ERR_INVALID, "No frames rendered yet");
        return nullptr;
    }
    *divisor = (float)frame_count;
    return c->accum;
}

// counts = the histogram of img[0..n) / divisor, waited for
int meter_image(spt_ctx* c, const char* who, const float4* img, uint64_t n, float divisor, uint32_t* counts) {
    SPT_HIP(c, hipSetDevice(c->device));
    if (const int rc = ensure_buf(c, c->meter_counts, SPT_METER_BINS, who); rc != SPT_OK) return rc;
    SPT_HIP(c, hipMemsetAsync(c->meter_counts, 0, sizeof(uint32_t) * SPT_METER_BINS, on_stream(c)));
    launch_meter(c->meter_form >= 0 ? c->meter_form : meter_default_form(), img, n, divisor, c->meter_counts, on_stream(c));
    SPT_HIP(c, hipGetLastError());
    SPT_HIP(c, hipMemcpyAsync(counts, c->meter_counts, sizeof(uint32_t) * SPT_METER_BINS, hipMemcpyDeviceToHost, on_stream(c)));
    SPT_HIP(c, hipStreamSynchronize(on_stream(c)));
    return SPT_OK;
}

float4 pixel_of(const float* a, uint64_t i) { return make_float4(a[4 * i], a[4 * i + 1], a[4 * i + 2], a[4 * i + 3]); }
}  // namespace

int spt_exposure_params_default(spt_exposure_params* out) {
    if (!out) return SPT_ERR_INVALID;
    *out = kExposureDefaults;
    return SPT_OK;
}

int spt_meter_luminance(spt_ctx* c, uint32_t image, uint32_t frame_count, uint32_t counts[SPT_METER_BINS]) {
    if (!c || !counts) return SPT_ERR_INVALID;
    float divisor = 1.0f;
    int rc = SPT_OK;
    const float4* img = display_source(c, image, frame_count, &divisor, &rc);
    if (!img) return rc;
    return meter_image(c, "spt_meter_luminance", img, c->pixels, divisor, counts);
}

int spt_meter_device_image(spt_ctx* c, const void* device_rgba, uint64_t n_pixels, float divisor,
                           uint32_t counts[SPT_METER_BINS]) {
    if (!c || !device_rgba || !counts) return SPT_ERR_INVALID;
    if (n_pixels == 0) return fail(c, SPT_ERR_INVALID, "spt_meter_device_image: no pixels");
    if (!divisor_ok(divisor)) return fail(c, SPT_ERR_INVALID, "spt_meter_device_image: divisor must be finite and > 0");
    return meter_image(c, "spt_meter_device_image", (const float4*)device_rgba, n_pixels, divisor, counts);
}

int spt_resolve_display_rgba8(spt_ctx* c, uint32_t image, uint32_t frame_count, const spt_display* display,
                              uint32_t* host_out) {
    if (!c || !display || !host_out) return SPT_ERR_INVALID;
    const spt_display d = *display;
    if (const char* msg = display_error(d)) return fail(c, SPT_ERR_INVALID, msg);
    float divisor = 1.0f;
    int rc = SPT_OK;
    const float4* img = display_source(c, image, frame_count, &divisor, &rc);
    if (!img) return rc;
    return resolve_image_by(c, host_out, [&](uint32_t* out, hipStream_t s) {
        launch_display(img, c->pixels, divisor, d, out, s);
    });
}

int spt_resolve_display_device_image(spt_ctx* c, const void* device_rgba, uint64_t n_pixels, float divisor,
                                     const spt_display* display, uint32_t* host_out) {
    if (!c || !device_rgba || !display || !host_out) return SPT_ERR_INVALID;
    if (n_pixels == 0) return fail(c, SPT_ERR_INVALID, "spt_resolve_display_device_image: no pixels");
    if (!divisor_ok(divisor))
        return fail(c, SPT_ERR_INVALID, "spt_resolve_display_device_image: divisor must be finite and > 0");
    const spt_display d = *display;
    if (const char* msg = display_error(d)) return fail(c, SPT_ERR_INVALID, msg);
    SPT_HIP(c, hipSetDevice(c->device));
    if (c->display_stage.size() < n_pixels) {
        SPT_HIP(c, hipStreamSynchronize(on_stream(c)));  // (no earlier resolve may still read the old one)
        if (!c->display_stage.ensure_at_least(n_pixels))
            return fail(c, SPT_ERR_HIP, "spt_resolve_display_device_image: allocation failed");
    }
    launch_display((const float4*)device_rgba, n_pixels, divisor, d, c->display_stage, on_stream(c));
    SPT_HIP(c, hipGetLastError());
    SPT_HIP(c, hipMemcpyAsync(host_out, c->display_stage, sizeof(uint32_t) * n_pixels, hipMemcpyDeviceToHost, on_stream(c)));
    SPT_HIP(c, hipStreamSynchronize(on_stream(c)));
    return SPT_OK;
}

int spt_set_meter_form(spt_ctx* c, int form) {
    if (!c) return SPT_ERR_INVALID;
    if (form != -1 && form != kMeterLanes && form != kMeterPeel)
        return fail(c, SPT_ERR_INVALID, "spt_set_meter_form: -1 (automatic), 0 (an add per lane) or 1 (an add per distinct bin)");
    c->meter_form = form;
    return SPT_OK;
}

int spt_meter_bin(float luminance, uint32_t* bin) {
    if (!bin) return SPT_ERR_INVALID;
    *bin = meter_bin(luminance);
    return SPT_OK;
}

int spt_luminance_histogram_host(const float* rgba, uint64_t n_pixels, float divisor, uint32_t counts[SPT_METER_BINS]) {
    if (!rgba || !counts || n_pixels == 0 || !divisor_ok(divisor)) return SPT_ERR_INVALID;
    std::memset(counts, 0, sizeof(uint32_t) * SPT_METER_BINS);
    for (uint64_t i = 0; i < n_pixels; ++i) counts[meter_bin(pixel_luminance(pixel_of(rgba, i), divisor))] += 1u;
    return SPT_OK;
}

int spt_exposure_from_histogram(const uint32_t counts[SPT_METER_BINS], const spt_exposure_params* params, float* exposure) {
    if (!counts || !exposure) return SPT_ERR_INVALID;
    const spt_exposure_params p = params ? *params : kExposureDefaults;
    if (!exposure_params_ok(p)) return SPT_ERR_INVALID;
    uint64_t total = 0;
    for (int b = 1; b < SPT_METER_BINS; ++b) total += counts[b];
    if (total == 0) {
        *exposure = 1.0f;
        return SPT_OK;
    }
    const double n = (double)total;
    const double lo = (double)p.low_fraction * n, hi = (1.0 - (double)p.high_fraction) * n;
    double c0 = 0.0, sw = 0.0, sl = 0.0;
    for (int b = 1; b < SPT_METER_BINS; ++b) {
        const double c1 = c0 + (double)counts[b];
        const double w = std::max(0.0, std::min(c1, hi) - std::max(c0, lo));
        const int key = kMeterKeyBase + b, e = (key >> 3) - 127, k = key & 7;
        const double centre = (double)e + std::log2(1.0 + ((double)k + 0.5) / 8.0);
        sw += w;
        sl += w * centre;
        c0 = c1;
    }
    double x = (double)p.target_luminance / std::exp2(sl / sw);
    x = std::min(std::max(x, (double)p.min_exposure), (double)p.max_exposure);
    *exposure = (float)x;
    return SPT_OK;
}

int spt_display_host(const float* rgba, uint64_t n_pixels, float divisor, const spt_display* display, uint32_t* out) {
    if (!rgba || !display || !out || n_pixels == 0 || !divisor_ok(divisor)) return SPT_ERR_INVALID;
    const spt_display d = *display;
    if (display_error(d)) return SPT_ERR_INVALID;
    for (uint64_t i = 0; i < n_pixels; ++i) out[i] = display_rgba8(pixel_of(rgba, i), divisor, d);
    return SPT_OK;
}

// ---- noise estimate: batch moments, the meter, the stop rule ------------------------------------------

namespace {
// counts and the e2 image (may be nullptr) of width x height device moments, waited for
int noise_meter_image(spt_ctx* c, const char* who, const float4* state, uint32_t width, uint32_t height, uint32_t batches,
                      float W, const spt_noise_params& p, uint32_t* counts, float* e2) {
    SPT_HIP(c, hipSetDevice(c->device));
    if (const int rc = ensure_buf(c, c->meter_counts, SPT_METER_BINS, who); rc != SPT_OK) return rc;
    SPT_HIP(c, hipMemsetAsync(c->meter_counts, 0, sizeof(uint32_t) * SPT_NOISE_BINS, on_stream(c)));
    launch_noise_meter(state, width, height, (int)p.radius, noise_inv(batches, W), p.dark_floor, c->meter_counts, e2, on_stream(c));
    SPT_HIP(c, hipGetLastError());
    SPT_HIP(c, hipMemcpyAsync(counts, c->meter_counts, sizeof(uint32_t) * SPT_NOISE_BINS, hipMemcpyDeviceToHost, on_stream(c)));
    SPT_HIP(c, hipStreamSynchronize(on_stream(c)));
    return SPT_OK;
}
static_assert(SPT_NOISE_BINS == SPT_METER_BINS, "the two meters share the ctx's 256 device words");
}  // namespace

int spt_noise_update(spt_ctx* c, uint32_t frame_count) {
    if (!c) return SPT_ERR_INVALID;
    if (!c->configured) return fail(c, SPT_ERR_NOT_CONFIGURED, "spt_noise_update before spt_configure");
    if (frame_count <= c->noise_frames) return fail(c, SPT_ERR_INVALID, "spt_noise_update: no frames since the last update");
    if (frame_count > (1u << 24)) return fail(c, SPT_ERR_INVALID, "spt_noise_update: more than 2^24 frames");
    SPT_HIP(c, hipSetDevice(c->device));
    const size_t pixels = std::max<size_t>(c->pixels, 1);
    if (const int rc = ensure_buf(c, c->noise_state, pixels, "spt_noise_update"); rc != SPT_OK) return rc;
    if (c->noise_batches == 0) SPT_HIP(c, hipMemsetAsync(c->noise_state, 0, sizeof(float4) * pixels, on_stream(c)));
    const float w = (float)(frame_count - c->noise_frames);
    launch_noise_update(c->accum, c->noise_state, c->pixels, noise_batch(w, c->noise_W), on_stream(c));
    SPT_HIP(c, hipGetLastError());
    c->noise_W = c->noise_W + w;
    c->noise_frames = frame_count;
    c->noise_batches += 1u;
    c->noise_metered = false;
    return SPT_OK;
}

int spt_noise_batches(const spt_ctx* c, uint32_t* batches, uint32_t* frames) {
    if (!c) return SPT_ERR_INVALID;
    if (batches) *batches = c->noise_batches;
    if (frames) *frames = c->noise_frames;
    return SPT_OK;
}

int spt_noise_meter(spt_ctx* c, const spt_noise_params* params, uint32_t counts[SPT_NOISE_BINS]) {
    if (!c || !counts) return SPT_ERR_INVALID;
    if (!c->configured) return fail(c, SPT_ERR_NOT_CONFIGURED, "spt_noise_meter before spt_configure");
    const spt_noise_params p = params ? *params : kNoiseDefaults;
    if (const char* msg = noise_params_error(p)) return fail(c, SPT_ERR_INVALID, msg);
    if (c->noise_batches < 2) return fail(c, SPT_ERR_INVALID, "spt_noise_meter: fewer than two updates since the accumulation restarted");
    if (p.radius > 0 && c->cfg.shard_count != 1u)
        return fail(c, SPT_ERR_INVALID, "spt_noise_meter: pooling (radius > 0) needs the whole image (shard_count 1)");
    SPT_HIP(c, hipSetDevice(c->device));
    if (c->pixels == 0) {
        std::memset(counts, 0, sizeof(uint32_t) * SPT_NOISE_BINS);
        return SPT_OK;
    }
    if (const int rc = ensure_buf(c, c->noise_e2, c->pixels, "spt_noise_meter"); rc != SPT_OK) return rc;
    const int rc = noise_meter_image(c, "spt_noise_meter", c->noise_state,c->cfg.width, c->rows, c->noise_batches, c->noise_W, p, counts, c->noise_e2);
    c->noise_metered = rc == SPT_OK;
    return rc;
}

int spt_read_noise_moments(spt_ctx* c, float* host_moments) {
    if (!c || !host_moments) return SPT_ERR_INVALID;
    if (!c->noise_state || c->noise_batches == 0) return fail(c, SPT_ERR_INVALID, "no noise moments: spt_noise_update first");
    SPT_HIP(c, hipSetDevice(c->device));
    if (c->pixels == 0) return SPT_OK;
    SPT_HIP(c, hipMemcpyAsync(host_moments, c->noise_state, sizeof(float4) * c->pixels, hipMemcpyDeviceToHost, on_stream(c)));
    SPT_HIP(c, hipStreamSynchronize(on_stream(c)));
    return SPT_OK;
}

int spt_read_noise(spt_ctx* c, float* host_e2) {
    if (!c || !host_e2) return SPT_ERR_INVALID;
    if (!c->noise_e2 || !c->noise_metered) return fail(c, SPT_ERR_INVALID, "no noise image: spt_noise_meter first");
    SPT_HIP(c, hipSetDevice(c->device));
    SPT_HIP(c, hipMemcpyAsync(host_e2, c->noise_e2, sizeof(float) * c->pixels, hipMemcpyDeviceToHost, on_stream(c)));
    SPT_HIP(c, hipStreamSynchronize(on_stream(c)));
    return SPT_OK;
}

int spt_noise_device_ptr(spt_ctx* c, void** moments, void** e2, uint64_t* pixels) {
    if (!c) return SPT_ERR_INVALID;
    if (!c->configured) return fail(c, SPT_ERR_NOT_CONFIGURED, "not configured");
    if (moments) *moments = c->noise_state;
    if (e2) *e2 = c->noise_e2;
    if (pixels) *pixels = c->pixels;
    return SPT_OK;
}

int spt_noise_meter_device_image(spt_ctx* c, const void* device_moments, uint32_t width, uint32_t height, uint32_t batches,
                                 float frames, const spt_noise_params* params, uint32_t counts[SPT_NOISE_BINS],
                                 void* device_e2) {
    if (!c || !device_moments || !counts) return SPT_ERR_INVALID;
    const spt_noise_params p = params ? *params : kNoiseDefaults;
    if (const char* msg = noise_params_error(p)) return fail(c, SPT_ERR_INVALID, msg);
    if (const char* msg = noise_image_error(width, height, batches, frames)) return fail(c, SPT_ERR_INVALID, msg);
    return noise_meter_image(c, "spt_noise_meter_device_image", (const float4*)device_moments, width, height, batches, frames, p, counts, (float*)device_e2);
}

int spt_camera_look_at(const float eye[3], const float target[3], const float up[3], float vfov_degrees,
                       spt_camera* out) {
    if (!eye || !target || !up || !out) return SPT_ERR_INVALID;
    if (!(vfov_degrees > 0.0f && vfov_degrees < 180.0f)) return SPT_ERR_INVALID;
    auto norm = [](double v[3]) {
        const double l = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
        if (!(l > 0.0) || !std::isfinite(l)) return false;
        for (int a = 0; a < 3; ++a) v[a] /= l;
        return true;
    };
    double f[3], r[3], t[3];
    for (int a = 0; a < 3; ++a) f[a] = (double)target[a] - (double)eye[a];
    if (!norm(f)) return SPT_ERR_INVALID;  // eye == target
    const double upd[3] = {up[0], up[1], up[2]};
    r[0] = upd[1] * f[2] - upd[2] * f[1];  // cross(up, f)
    r[1] = upd[2] * f[0] - upd[0] * f[2];
    r[2] = upd[0] * f[1] - upd[1] * f[0];
    // up parallel to the view direction: |cross| vanishes against |up| (|f| = 1)
    const double ul = std::sqrt(upd[0] * upd[0] + upd[1] * upd[1] + upd[2] * upd[2]);
    const double rl = std::sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
    if (!(ul > 0.0) || !std::isfinite(ul) || !(rl > 1e-12 * ul)) return SPT_ERR_INVALID;
    if (!norm(r)) return SPT_ERR_INVALID;
    t[0] = f[1] * r[2] - f[2] * r[1];  // cross(f, r)
    t[1] = f[2] * r[0] - f[0] * r[2];
    t[2] = f[0] * r[1] - f[1] * r[0];
    // tan(vfov / 2); 90 degrees is exactly 1 (tan(pi / 4) in double is 1 - 1 ulp)
    const double h = vfov_degrees == 90.0f ? 1.0 : std::tan((double)vfov_degrees * (3.14159265358979323846 / 360.0));
    spt_camera cam{};
    for (int a = 0; a < 3; ++a) {
        cam.origin[a] = eye[a];
        cam.u[a] = (float)(r[a] * h);
        cam.v[a] = (float)(t[a] * h);
        cam.w[a] = (float)f[a];
    }
    *out = cam;
    return SPT_OK;
}

int spt_camera_ray(const spt_camera* cam, uint32_t width, uint32_t height, uint32_t x, uint32_t y, float jx, float jy,
                   float o[3], float d[3]) {
    if (!cam || !o || !d || width == 0 || height == 0) return SPT_ERR_INVALID;
    const CameraPose pose{F3{cam->origin[0], cam->origin[1], cam->origin[2]}, F3{cam->u[0], cam->u[1], cam->u[2]},
                          F3{cam->v[0], cam->v[1], cam->v[2]}, F3{cam->w[0], cam->w[1], cam->w[2]}};
    // the constants base_params computes (CPUPathTracer.cpp:53-54, 65)
    const F3 dir = camera_ray_dir(pose, x, y, jx, jy, 1.0f / (float)width, 1.0f / (float)height,
                                  (float)width / (float)height);
    for (int a = 0; a < 3; ++a) o[a] = cam->origin[a];
    d[0] = dir.x;
    d[1] = dir.y;
    d[2] = dir.z;
    return SPT_OK;
}

int spt_camera_lens_ray(const spt_camera* cam, const spt_lens* lens, uint32_t width, uint32_t height, uint32_t x,
                        uint32_t y, float jx, float jy, float u1, float u2, float o[3], float d[3]) {
    if (!cam || !lens || !o || !d || width == 0 || height == 0) return SPT_ERR_INVALID;
    if (lens_error(*lens)) return SPT_ERR_INVALID;
    // the aperture sample is a pair of random_float values: sincos_2pi is stated for phi in [0, 2 pi]
    if (!(u1 >= 0.0f && u1 <= 1.0f) || !(u2 >= 0.0f && u2 <= 1.0f)) return SPT_ERR_INVALID;
    const CameraPose pose{F3{cam->origin[0], cam->origin[1], cam->origin[2]}, F3{cam->u[0], cam->u[1], cam->u[2]},
                          F3{cam->v[0], cam->v[1], cam->v[2]}, F3{cam->w[0], cam->w[1], cam->w[2]}};
    F3 org;
    const F3 dir = camera_lens_ray(pose, lens_scalars(*cam, *lens), x, y, jx, jy, u1, u2, 1.0f / (float)width,
                                   1.0f / (float)height, (float)width / (float)height, org);
    o[0] = org.x;
    o[1] = org.y;
    o[2] = org.z;
    d[0] = dir.x;
    d[1] = dir.y;
    d[2] = dir.z;
    return SPT_OK;
}

int spt_camera_focus_at_hit(const spt_camera* cam, uint32_t width, uint32_t height, uint32_t x, uint32_t y, float jx,
                            float jy, float t, float* focus_distance) {
    if (!cam || !focus_distance || width == 0 || height == 0) return SPT_ERR_INVALID;
    if (!std::isfinite(t) || !(t > 0.0f)) return SPT_ERR_INVALID;
    // |p| of the pixel's image-plane vector, the formula of camera_ray_dir in double
    const double px = (double)x + (double)jx, py = (double)y + (double)jy;
    const double sx = ((px / (double)width) * 2.0 - 1.0) * ((double)width / (double)height);
    const double sy = (1.0 - py / (double)height) * 2.0 - 1.0;
    double q = 0.0;
    for (int a = 0; a < 3; ++a) {
        const double p = (sx * (double)cam->u[a] + sy * (double)cam->v[a]) + (double)cam->w[a];
        q += p * p;
    }
    const double len = std::sqrt(q);
    if (!(len > 0.0) || !std::isfinite(len)) return SPT_ERR_INVALID;
    *focus_distance = (float)((double)t / len);
    return SPT_OK;
}

int spt_env_octa_from_equirect(const float* src, uint32_t sw, uint32_t sh, float* dst, uint32_t dw, uint32_t dh) {
    if (!src || !dst || sw == 0 || sh == 0 || dw == 0 || dh == 0) return SPT_ERR_INVALID;
    const double kPi = 3.14159265358979323846;
    for (uint32_t iy = 0; iy < dh; ++iy) {
        for (uint32_t ix = 0; ix < dw; ++ix) {
            // octahedral decode of the texel centre (the inverse of octa_texel's projection)
            double px = 2.0 * (ix + 0.5) / dw - 1.0, pz = 2.0 * (iy + 0.5) / dh - 1.0;
            double y = 1.0 - std::fabs(px) - std::fabs(pz);
            if (y < 0.0) {
                const double fx = (1.0 - std::fabs(pz)) * (px >= 0.0 ? 1.0 : -1.0);
                const double fz = (1.0 - std::fabs(px)) * (pz >= 0.0 ? 1.0 : -1.0);
                px = fx;
                pz = fz;
            }
            const double len = std::sqrt(px * px + y * y + pz * pz);
            const double x = px / len, yy = y / len, z = pz / len;
            const double phi = std::atan2(x, -z);                              // [-pi, pi]
            const double theta = std::acos(std::max(-1.0, std::min(1.0, yy)));  // 0 at +y
            uint32_t sx = (uint32_t)((phi + kPi) / (2.0 * kPi) * sw), sy = (uint32_t)(theta / kPi * sh);
            sx = std::min(sx, sw - 1u);
            sy = std::min(sy, sh - 1u);
            const float* t = src + 3ull * ((size_t)sy * sw + sx);
            float* o = dst + 4ull * ((size_t)iy * dw + ix);
            o[0] = t[0];
            o[1] = t[1];
            o[2] = t[2];
            o[3] = 1.0f;
        }
    }
    return SPT_OK;
}

int spt_set_profiling(spt_ctx* c, int mode) {
    if (!c) return SPT_ERR_INVALID;
    SPT_HIP(c, hipSetDevice(c->device));
    const bool span = (mode & SPT_PROFILE_SPAN) != 0;
    if (!span && close_span(c) != SPT_OK) return SPT_ERR_HIP;  // (recorded before any flush waits)
    if (!(mode & (SPT_PROFILE_EVENTS | SPT_PROFILE_SPAN)) && flush_events(c) != SPT_OK) return SPT_ERR_HIP;
    c->profiling = (mode & (SPT_PROFILE_EVENTS | SPT_PROFILE_SPAN)) != 0;
    c->span = span;
    const bool counters = (mode & SPT_PROFILE_COUNTERS) != 0;
    // (frame_lists_scene: the counting kernels never hold a scene in LDS, so the lists are decided again)
    if (counters != c->counters) c->derived.drop(Change::Counters);
    c->counters = counters;
    return SPT_OK;
}

int spt_get_stats(spt_ctx* c, spt_stats* out) {
    if (!c || !out) return SPT_ERR_INVALID;
    SPT_HIP(c, hipSetDevice(c->device));
    SPT_HIP(c, hipStreamSynchronize(on_stream(c)));
    if (flush_events(c) != SPT_OK) return SPT_ERR_HIP;
    unsigned long long tot[kTotals];
    SPT_HIP(c, hipMemcpy(tot, c->totals, sizeof(tot), hipMemcpyDeviceToHost));
    std::memset(out, 0, sizeof(*out));
    out->frames = c->frames;
    out->paths = c->paths;
    out->passes = c->passes;
    for (uint32_t b = 0; b < kMaxBounces && b < SPT_MAX_BOUNCES; ++b) {
        out->segments[b] = tot[b];
        out->segments_total += tot[b];
        out->radiance_updates[b] = tot[kMaxBounces + b];
    }
    out->extend_launches = c->ext_launches;
    out->extend_ms = c->ext_ms;
    out->extend_segments = c->ext_launches ? out->segments_total : 0;
    out->shade_launches = c->shade_launches;
    out->shade_ms = c->shade_ms;
    out->other_ms = c->other_ms;
    out->tail_ms = c->tail_ms;
    out->tail_launches = c->tail_launches;
    out->tail_bounce = schedule_tail(c);
    out->fused = schedule_fused(c) ? 1u : 0u;
    out->persistent_ms = c->persist_ms;
    out->persistent_launches = c->persist_launches;
    out->schedule = c->last_schedule;
    out->lane_slots = tot[2 * kMaxBounces];
    out->lane_busy = tot[2 * kMaxBounces + 1];
    out->bvh_node_visits = tot[2 * kMaxBounces + 2];
    out->prim_tests = tot[2 * kMaxBounces + 3];
    out->flat_fast_path = (c->fast_div && c->n_prims <= kFlatSceneMax) ? 1u : 0u;
    out->specialized = c->last_specialized ? 1u : 0u;
    for (uint32_t b = 0; b < kMaxBounces && b < SPT_MAX_BOUNCES; ++b) {
        out->extend_ms_bounce[b] = c->ext_ms_b[b];
        out->shade_ms_bounce[b] = c->shade_ms_b[b];
    }
    out->bvh_nodes = c->n_nodes;
    out->scene_bytes = c->scene_bytes;
    out->shadow_rays = tot[kTotShadow];
    out->emitters = c->n_emit;
    out->stack_bytes = c->stack_bytes;
    out->stack_need = c->bvh_stack_need;
    out->stalled_waves = tot[kTotStalled];
    out->view_cached = c->last_view_cached ? 1u : 0u;
    out->view_live_pixels = c->derived.valid(kViewLists) ? c->view_n[0] : 0u;
    out->flat_pairs = c->last_specialized ? c->last_pairs : 0u;
    out->flat_pair_second_passes = tot[kTotPairSecond];
    out->flat_sphere_second_passes = tot[kTotSphereSecond];
    out->view_split = c->last_view_split ? 1u : 0u;
    if (tot[kTotStalled])
        return fail(c, SPT_ERR_HIP, "k_paths: " + std::to_string(tot[kTotStalled]) +
                                        " wave(s) stopped at the step bound with frames unaccumulated (a bug)");
    return SPT_OK;
}

int spt_get_view_wide(spt_ctx* c, uint64_t* view_wide) {
    if (!c || !view_wide) return SPT_ERR_INVALID;
    *view_wide = c->last_view_wide ? 1u : 0u;
    return SPT_OK;
}

int spt_get_flat_ranges(spt_ctx* c, uint64_t* flat_ranges) {
    if (!c || !flat_ranges) return SPT_ERR_INVALID;
    *flat_ranges = c->last_ranges ? 1u : 0u;
    return SPT_OK;
}

int spt_stats_clear(spt_ctx* c) {
    if (!c) return SPT_ERR_INVALID;
    SPT_HIP(c, hipSetDevice(c->device));
    SPT_HIP(c, hipStreamSynchronize(on_stream(c)));
    if (flush_events(c) != SPT_OK) return SPT_ERR_HIP;
    SPT_HIP(c, hipMemset(c->totals, 0, sizeof(unsigned long long) * kTotals));
    c->frames = c->paths = c->passes = 0;
    c->ext_launches = c->shade_launches = c->ext_segments = 0;
    c->ext_ms = c->shade_ms = c->other_ms = c->tail_ms = 0.0;
    c->tail_launches = 0;
    c->persist_ms = 0.0;
    c->persist_launches = 0;
    for (uint32_t b = 0; b < kMaxBounces; ++b) c->ext_ms_b[b] = c->shade_ms_b[b] = 0.0;
    return SPT_OK;
}

int spt_specialize_scene(spt_ctx* c) {
    if (!c) return SPT_ERR_INVALID;
    if (!c->has_scene) return fail(c, SPT_ERR_NO_SCENE, "spt_specialize_scene before spt_set_scene");
    if (c->n_prims == 0 || c->n_nodes != 0 || c->specialize < 0) return SPT_OK;  // nothing to specialize
    SPT_HIP(c, hipSetDevice(c->device));
    const uint64_t key = flat_jit_key(c);  // (before spt_configure: the shape alone)
    std::string err;
    const JitFormList forms = jit_kinds_of_scene(nee_active(c), c->d_env ? 1 : 0, wide_possible_ctx(c));
    for (int i = 0; i < forms.n; ++i)
        if (!jit_function(forms.f[i], key, &err))
            return fail(c, SPT_ERR_HIP, ("specialized kernels unavailable (the generic ones run): " + err).c_str());
    return SPT_OK;
}

int spt_compile_flat_kernels(const spt_prim* prims, uint32_t n_prims, int env_map, char* log, size_t log_bytes) {
    if (log && log_bytes) log[0] = 0;
    if ((!prims && n_prims) || n_prims == 0 || n_prims > kFlatSceneMax) return SPT_ERR_INVALID;
    uint32_t n_mats = 1;
    for (uint32_t i = 0; i < n_prims; ++i) n_mats = std::max(n_mats, prims[i].material + 1u);
    std::vector<DevPrim> dp, sorted;
    const char* msg = nullptr;
    if (!prepare_prims(prims, n_prims, n_mats, dp, &msg)) return SPT_ERR_INVALID;
    uint32_t ends[kFlatKinds - 1], flat_ends = 0;
    sort_flat_by_kind(dp, sorted, ends);
    for (uint32_t g = 0; g + 1 < kFlatKinds; ++g) flat_ends |= ends[g] << (6 * g);
    const uint32_t flat_rect = flat_rect_bits(sorted, ends);
    const uint64_t key = flat_shape_key(flat_ends, n_prims, flat_rect, flat_wall_pairs(sorted, ends, flat_rect));
    std::string out;
    const JitFormList forms = jit_kinds_of_scene(false, env_map ? 1 : 0);  // (no emitters known here: the forms without NEE)
    int built = 0;
    while (built < forms.n && jit_compile(forms.f[built], key, &out)) ++built;
    if (built == forms.n) return SPT_OK;
    if (log && log_bytes) {
        std::strncpy(log, out.c_str(), log_bytes - 1);
        log[log_bytes - 1] = 0;
    }
    return SPT_ERR_HIP;
}

int spt_set_tuning(spt_ctx* c, const spt_tuning* t) {
    if (!c || !t) return SPT_ERR_INVALID;
    if (t->fused < -1 || t->fused > 1 || t->persistent < -1 || t->persistent > 1 || t->frame_kernel < -1 ||
        t->frame_kernel > 1)
        return fail(c, SPT_ERR_INVALID, "spt_tuning: fused / persistent / frame_kernel must be -1, 0 or 1");
    if (t->px_shift && (t->px_shift < 2 || t->px_shift > 5)) return fail(c, SPT_ERR_INVALID, "spt_tuning: px_shift 2..5");
    if (t->chunks_per_wave > 1024 || t->subqueues > 65536 || t->tail_bounce > kMaxBounces ||
        t->bvh_max_leaf > kBvhMaxLeaf || (t->bvh_bins && (t->bvh_bins < 2 || t->bvh_bins > 64)) ||
        t->specialize < -1 || t->specialize > 1 || t->view_cache < -1 || t->view_cache > 0 || t->split_streams < -1 ||
        t->split_streams > 1 || t->wide_chunks < -1 || t->wide_chunks > 1)
        return fail(c, SPT_ERR_INVALID, "spt_tuning: value out of range");
    SPT_HIP(c, hipSetDevice(c->device));
    SPT_HIP(c, hipStreamSynchronize(on_stream(c)));
    const uint32_t n_sub = t->subqueues ? t->subqueues : c->cu_count * 12u;
    if (n_sub != c->n_sub) {  // the wavefront schedule's per-sub-queue counters: the new buffer first,
        // swapped in only once it exists (a failed allocation leaves the ctx as it was)
        Dev<uint32_t> counts;
        if (!counts.alloc((size_t)2 * (kMaxBounces + 1) * n_sub)) return fail(c, SPT_ERR_HIP, "spt_set_tuning: allocation failed");
        if (hipMemset(counts, 0, sizeof(uint32_t) * counts.size()) != hipSuccess)
            return fail(c, SPT_ERR_HIP, "spt_set_tuning: hipMemset of the sub-queue counters failed");
        c->counts.swap(counts);
        c->n_sub = n_sub;
    }
    c->fused_override = t->fused;
    c->tail_override = t->tail_bounce;
    c->persistent_override = t->persistent;
    c->frame_override = t->frame_kernel;
    c->chunks_per_wave = t->chunks_per_wave;
    c->px_shift = t->px_shift;
    c->bvh_max_leaf = t->bvh_max_leaf;
    c->bvh_bins = t->bvh_bins;
    c->specialize = t->specialize;
    c->view_cache = t->view_cache;
    c->split_streams = t->split_streams;
    c->wide_chunks = t->wide_chunks;
    return SPT_OK;
}

int spt_comm_available(void) { return rccl().ok ? SPT_OK : SPT_ERR_NO_DEVICE; }

int spt_comm_unique_id(uint8_t id[SPT_COMM_ID_BYTES]) {
    static_assert(sizeof(ncclUniqueId) == SPT_COMM_ID_BYTES, "RCCL unique id size");
    if (!id) return SPT_ERR_INVALID;
    if (!rccl().ok) return SPT_ERR_NO_DEVICE;
    ncclUniqueId u;
    if (rccl().get_unique_id(&u) != ncclSuccess) return SPT_ERR_HIP;
    std::memcpy(id, &u, sizeof(u));
    return SPT_OK;
}

int spt_comm_init(spt_ctx* c, const uint8_t id[SPT_COMM_ID_BYTES], int n_ranks, int rank) {
    if (!c || !id) return SPT_ERR_INVALID;
    if (n_ranks < 1 || rank < 0 || rank >= n_ranks) return fail(c, SPT_ERR_INVALID, "spt_comm_init: rank out of range");
    if (!rccl().ok) return fail(c, SPT_ERR_NO_DEVICE, rccl().err);
    SPT_HIP(c, hipSetDevice(c->device));
    SPT_HIP(c, hipStreamSynchronize(on_stream(c)));
    free_comm(c);
    ncclUniqueId u;
    std::memcpy(&u, id, sizeof(u));
    SPT_NCCL(c, rccl().comm_init_rank(&c->comm, n_ranks, u, rank));
    c->comm_ranks = n_ranks;
    c->comm_rank = rank;
    return SPT_OK;
}

int spt_comm_destroy(spt_ctx* c) {
    if (!c) return SPT_ERR_INVALID;
    SPT_HIP(c, hipSetDevice(c->device));
    SPT_HIP(c, hipStreamSynchronize(on_stream(c)));
    free_comm(c);
    return SPT_OK;
}

namespace {
// Checks shared by both gathers; rows_max / shard_elems: the padded shard's rows and floats.
int gather_check(spt_ctx* c, void* root_image, const char* what, uint32_t& rows_max, size_t& shard_elems) {
    if (!c->configured) return fail(c, SPT_ERR_NOT_CONFIGURED, "not configured");
    if (!c->comm) return fail(c, SPT_ERR_INVALID, std::string(what) + " before spt_comm_init");
    const uint32_t world = c->cfg.shard_count;
    if ((int)world != c->comm_ranks || (int)c->cfg.shard_rank != c->comm_rank)
        return fail(c, SPT_ERR_INVALID, std::string(what) + ": shard_rank / shard_count differ from the communicator's rank / size");
    if (c->comm_rank == 0 && !root_image) return fail(c, SPT_ERR_INVALID, std::string(what) + ": rank 0 needs an output image");
    SPT_HIP(c, hipSetDevice(c->device));
    rows_max = (c->cfg.height + world - 1) / world;
    shard_elems = (size_t)rows_max * c->cfg.width * 4;
    return SPT_OK;
}

// gather_buf of `need` floats, its padding rows zeroed once (every copy into it writes the same rows)
int gather_buffer(spt_ctx* c, size_t need) {
    const size_t texels = need / 4;  // (a shard is whole pixels)
    if (c->gather_buf.size() == texels) return SPT_OK;
    if (c->gather_pending) SPT_HIP(c, hipStreamWaitEvent(on_stream(c), c->gather_done, 0));
    SPT_HIP(c, hipStreamSynchronize(on_stream(c)));  // (an earlier gather may still read the old buffer)
    // exactly the size, not the scratch's "at least": another size is another layout, whose padding rows are zero
    // only in a buffer zeroed for it
    if (!c->gather_buf.alloc(texels)) return fail(c, SPT_ERR_HIP, "spt_gather_image: allocation failed");
    if (texels) SPT_HIP(c, hipMemsetAsync(c->gather_buf, 0, sizeof(float4) * texels, on_stream(c)));
    return SPT_OK;
}
}  // namespace

int spt_gather_image(spt_ctx* c, void* root_image) {
    if (!c) return SPT_ERR_INVALID;
    uint32_t rows_max = 0;
    size_t shard_elems = 0;
    int st = gather_check(c, root_image, "spt_gather_image", rows_max, shard_elems);
    if (st != SPT_OK) return st;
    // rank 0 receives world padded shards; a rank owning fewer than rows_max rows sends from a
    // zero-padded copy of its shard, the others straight from the accumulation buffer
    const bool root = c->comm_rank == 0;
    const bool padded = c->rows < rows_max;
    st = gather_buffer(c, root ? shard_elems * c->cfg.shard_count : (padded ? shard_elems : 0));
    if (st != SPT_OK) return st;
    if (c->gather_pending) SPT_HIP(c, hipStreamWaitEvent(on_stream(c), c->gather_done, 0));  // gather_buf is free
    const float4* send = c->accum;
    if (padded && !root) {
        if (c->pixels)
            SPT_HIP(c, hipMemcpyAsync(c->gather_buf, c->accum, sizeof(float4) * c->pixels, hipMemcpyDeviceToDevice, on_stream(c)));
        send = c->gather_buf;
    }
    // one ncclGather for any world size (a 1-rank communicator copies: the single-GPU test runs the
    // same collective call the N-GPU run does)
    SPT_NCCL(c, rccl().gather(send, root ? c->gather_buf : nullptr, shard_elems, ncclFloat32, 0, c->comm, on_stream(c)));
    if (root) {
        launch_assemble_rows(c->gather_buf, (float4*)root_image, c->cfg.width, c->cfg.height, c->cfg.shard_count,
                             rows_max, on_stream(c));
        SPT_HIP(c, hipGetLastError());
    }
    return SPT_OK;
}

int spt_gather_image_overlapped(spt_ctx* c, void* root_image) {
    if (!c) return SPT_ERR_INVALID;
    uint32_t rows_max = 0;
    size_t shard_elems = 0;
    int st = gather_check(c, root_image, "spt_gather_image_overlapped", rows_max, shard_elems);
    if (st != SPT_OK) return st;
    const bool root = c->comm_rank == 0;
    st = gather_buffer(c, root ? shard_elems * c->cfg.shard_count : shard_elems);  // every rank sends a snapshot
    if (st != SPT_OK) return st;
    if (!c->comm_stream) {
        SPT_HIP(c, hipStreamCreateWithFlags(&c->comm_stream, hipStreamNonBlocking));
        SPT_HIP(c, hipEventCreateWithFlags(&c->snap_ready, hipEventDisableTiming));
        SPT_HIP(c, hipEventCreateWithFlags(&c->gather_done, hipEventDisableTiming));
    }
    // the snapshot, on the ctx stream after the frames rendered so far: rank 0's own shard goes to its
    // slot of the receive buffer (an in-place gather), the others' to their send buffer. The previous
    // overlapped gather must have finished reading that buffer first.
    if (c->gather_pending) SPT_HIP(c, hipStreamWaitEvent(on_stream(c), c->gather_done, 0));
    if (c->pixels)
        SPT_HIP(c, hipMemcpyAsync(c->gather_buf, c->accum, sizeof(float4) * c->pixels, hipMemcpyDeviceToDevice, on_stream(c)));
    SPT_HIP(c, hipEventRecord(c->snap_ready, on_stream(c)));
    // the collective and the assembly on the comm stream: the ctx stream renders on meanwhile
    SPT_HIP(c, hipStreamWaitEvent(c->comm_stream, c->snap_ready, 0));
    SPT_NCCL(c, rccl().gather(c->gather_buf, root ? c->gather_buf : nullptr, shard_elems, ncclFloat32, 0, c->comm,
                              c->comm_stream));
    if (root) {
        launch_assemble_rows(c->gather_buf, (float4*)root_image, c->cfg.width, c->cfg.height, c->cfg.shard_count,
                             rows_max, c->comm_stream);
        SPT_HIP(c, hipGetLastError());
    }
    SPT_HIP(c, hipEventRecord(c->gather_done, c->comm_stream));
    c->gather_pending = true;
    return SPT_OK;
}

int spt_gather_wait(spt_ctx* c) {
    if (!c) return SPT_ERR_INVALID;
    if (!c->gather_pending) return SPT_OK;
    SPT_HIP(c, hipSetDevice(c->device));
    SPT_HIP(c, hipStreamWaitEvent(on_stream(c), c->gather_done, 0));
    c->gather_pending = false;
    return SPT_OK;
}

}  // extern "C"
