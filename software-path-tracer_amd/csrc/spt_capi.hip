// spt_capi.hip — the C-ABI of libspt_hip.so (declared in include/spt.h): the context (spt_ctx.h). Its
// post-processing entry points are in spt_capi_post.hip, the entry points that take no context in spt_host.cpp.
// Owns one HIP device's state for the integrator: scene records, ray queues, accumulation, and
// the pass driver that replaces CPUPathTracer::render()'s serial pixel loop
// (libs/render/src/engines/pathtracer/backends/cpu/CPUPathTracer.cpp:43-85) with wavefront
// launches. Never aborts: every failure is a negative spt_status + spt_last_error().
#include <dlfcn.h>

#include <algorithm>
#include <cmath>
#include <cstring>

#include "spt_ctx.h"
#include "spt_device.h"
#include "spt_jit.h"
#include "spt_launch_plan.h"
#include "spt_params.h"

using namespace spt;

static_assert(kBvhStackMax == kBvhStackEntries, "scene.h and spt_kernels.h stack bounds");
static_assert(kMatDiffuse == SPT_MAT_DIFFUSE && kMatMetal == SPT_MAT_METAL && kMatDielectric == SPT_MAT_DIELECTRIC,
              "spt.h spt_material_kind and spt_device.h model_kind");
static_assert(sizeof(spt_material_model) == 16, "spt_material_model is 16 bytes");

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

// float4s in n records of a device array the kernels address as float4 (scene.h DevPrim, DevMaterial, DevEmitter)
template <class Rec>
size_t float4s(size_t n) {
    static_assert(sizeof(Rec) % sizeof(float4) == 0, "a device record is whole float4s");
    return n * (sizeof(Rec) / sizeof(float4));
}
static_assert(kDevNodeBytes % sizeof(float4) == 0, "a device node is whole float4s");

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


// The model word of a material (spt_device.h model_kind): +0.0f DIFFUSE, -fuzz METAL, ior DIELECTRIC.
float model_word(const spt_material_model& m) {
    if (m.kind == SPT_MAT_METAL) return -std::fabs(m.param);  // (a fuzz of -0.0f is a mirror too, not word 0)
    return m.kind == SPT_MAT_DIELECTRIC ? m.param : 0.0f;
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

PassParams spt::base_params(spt_ctx* c) {
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

// No context and no device call, but through spt_device.h (its host build needs the HIP compiler), so not in
// spt_host.cpp: spt_bsdf_sample, and below spt_camera_ray, spt_camera_lens_ray and spt_camera_focus_at_hit.
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
