/*
 * spt.h — C-ABI of libspt_hip.so, the MI355X (gfx950) path-tracing integrator.
 *
 * This is the drop-in boundary for the one hot path of imisumi/software-path-tracer:
 * the per-pixel integrator of render::CPUPathTracer
 *   (reference: libs/render/src/engines/pathtracer/backends/cpu/CPUPathTracer.cpp:43-326).
 * The C++ backend render::HIPPathTracer (software-path-tracer_amd/csrc/HIPPathTracer.cpp)
 * implements the reference's render::PathTracer interface (libs/render/include/render/PathTracer.h:13-51)
 * on top of these entry points; Python (ctypes) and any other FFI bind the same symbols.
 *
 * Conventions:
 *   - every int-returning call returns SPT_OK (0) on success and a negative spt_status otherwise;
 *     spt_last_error(ctx) gives the message. No call aborts: the C++ wrapper turns failures into
 *     the reference's fail-stop verify() (render_assert.h:15-25).
 *   - all arrays are plain POD owned by the caller; the ctx copies what it keeps.
 *   - a ctx is single-threaded (the reference calls its backend from App's main thread only,
 *     App.cpp:231-232) and bound to one HIP device. Multi-GPU = one ctx per process/GPU, each
 *     rendering an interleaved row shard (spt_config.shard_rank / shard_count); the shards are
 *     gathered to rank 0 over RCCL by spt_gather_image.
 *   - no torch / HIP types in signatures; a HIP stream is passed as an opaque void*.
 */
#ifndef SPT_H
#define SPT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SPT_ABI_VERSION 3  /* 3: SPT_FLAG_NEE, spt_stats.shadow_rays / emitters */

typedef enum spt_status {
    SPT_OK = 0,
    SPT_ERR_INVALID = -1,     /* bad argument / call order                                   */
    SPT_ERR_HIP = -2,         /* HIP runtime error (message in spt_last_error)              */
    SPT_ERR_NO_DEVICE = -3,   /* no gfx950 device / HIP runtime unusable                    */
    SPT_ERR_NO_SCENE = -4,    /* render before spt_set_scene (CPUPathTracer.cpp:46 verify)   */
    SPT_ERR_NOT_CONFIGURED = -5,
    SPT_ERR_CAPACITY = -6     /* caller buffer too small                                    */
} spt_status;

/* ---- scene input (replaces the Embree geometry of CPUPathTracer.cpp:328-404) ---------------- */

typedef enum spt_prim_type {
    SPT_PRIM_SPHERE = 0,   /* reference type: RTC_GEOMETRY_TYPE_SPHERE_POINT (CPUPathTracer.cpp:374) */
    SPT_PRIM_QUAD = 1,     /* superset: parallelogram Q + a*u + b*v, a,b in [0,1]                     */
    SPT_PRIM_TRIANGLE = 2  /* superset: (v0, v1, v2)                                                  */
} spt_prim_type;

/* 64-byte input record. Sphere: p0 = (cx, cy, cz, r) exactly the Embree FLOAT4 vertex
 * (CPUPathTracer.cpp:377-384). Quad: p0.xyz = Q, p1.xyz = u, p2.xyz = v.
 * Triangle: p0.xyz, p1.xyz, p2.xyz = v0, v1, v2. Unused lanes must be 0. */
typedef struct spt_prim {
    uint32_t type;       /* spt_prim_type                           */
    uint32_t material;   /* index into the material array           */
    uint32_t reserved[2];
    float p0[4];
    float p1[4];
    float p2[4];
} spt_prim;

/* Reference mode: every surface has albedo 0.7 (CPUPathTracer.cpp:260) and no emission. */
typedef struct spt_material {
    float albedo[3];
    float emission[3];
} spt_material;

/* Sky on miss: L += T * mix(horizon, zenith, 0.5*(d.y+1))  (CPUPathTracer.cpp:231-235, 286-292).
 * Reference values: horizon (1,1,1), zenith (0.5,0.7,1.0). */
typedef struct spt_env {
    uint32_t sky_enabled;
    float horizon[3];
    float zenith[3];
} spt_env;

/* ---- render configuration (RenderSettings, Types.h:43-95, as CPUPathTracer actually uses it) -- */

enum spt_flags {
    /* get_random_bounche's `abs(normal.z)` (CPUPathTracer.cpp:320) binds to ::abs(int) under
     * libstdc++ (the reference's Linux build); set this flag for the intended float fabs. */
    SPT_FLAG_ABS_FLOAT = 1u << 0,
    /* Schedule: trace each bounce as a separate closest-hit (k_extend) and shading (k_shade) launch
     * instead of the default fused bounce kernel. Same results; exposes the traversal kernel alone. */
    SPT_FLAG_SPLIT_KERNELS = 1u << 1,
    /* Schedule: keep the wavefront (queue) schedule instead of the persistent launches
     * (k_paths for calls of >= SPT_PERSISTENT_MIN_FRAMES frames, k_frame per frame below). */
    SPT_FLAG_WAVEFRONT = 1u << 2,
    /* Schedule (BVH scenes): the split wavefront with sorted ray queues — before every bounce >= 1
     * closest-hit launch the queued rays are binned by (direction octant, cell of the origin in an
     * 8x8x8 grid over the scene bounds) with a device counting sort and traced in bin order, so
     * neighbouring lanes and waves walk the same subtrees. Same results. Implies SPT_FLAG_WAVEFRONT
     * and SPT_FLAG_SPLIT_KERNELS. */
    SPT_FLAG_SORTED_RAYS = 1u << 3,
    /* Integrator (superset, SURVEY.md §8a.6, north_star "BRDF + light sampling"; the reference's bounce
     * loop, CPUPathTracer.cpp:229-281, has none): next-event estimation. At every hit that continues
     * (bounce_count < max_bounces, before Russian roulette) one point is sampled on the scene's emitters
     * — the quads, triangles and spheres whose material emits, in primitive order, chosen uniformly; a
     * point uniform over the chosen one's area — and a shadow ray from the offset hit point tests it; if
     * nothing lies in [0.001, 0.999 * distance) the Lambertian estimate T * Le * cos_s * cos_l * area *
     * n_emitters / (pi * distance^2) is added (a sphere's cos_l counts its side facing the hit point
     * only; quads and triangles emit from both sides). Emission reached by a BSDF ray then counts on
     * the camera segment only (with material models: also after a METAL or DIELECTRIC vertex, which takes
     * no light sample; see "materials" below).
     * RNG draw order per hit: emitter, u, v (NEE), then Russian roulette, then the direction.
     * oracle/cpu_ref.c restates it (ref_light_sample); every schedule gives identical results. */
    SPT_FLAG_NEE = 1u << 4
};

/* Which schedule spt_render used (spt_stats.schedule); every schedule gives identical results. */
enum spt_schedule {
    SPT_SCHEDULE_SPLIT = 0,      /* per bounce: k_extend + k_shade launches (BVH scenes)          */
    SPT_SCHEDULE_FUSED = 1,      /* per bounce: one k_shade<fused> launch, then k_trace_tail      */
    SPT_SCHEDULE_PERSISTENT = 2, /* one k_paths launch per call (per 1024 frames)                 */
    SPT_SCHEDULE_FRAME = 3       /* one k_frame launch per frame (calls of < 4 frames)            */
};
#define SPT_PERSISTENT_MIN_FRAMES 4

typedef struct spt_config {
    uint32_t width;             /* image width  (RenderSettings::getWidth,  CPUPathTracer.cpp:140) */
    uint32_t height;            /* image height                                                     */
    uint32_t max_bounces;       /* reference: hard-coded 4 (CPUPathTracer.cpp:199)                  */
    uint32_t rr_depth;          /* RR when bounce_count > rr_depth; reference: 2 (:264)             */
    uint32_t flags;             /* spt_flags                                                         */
    uint32_t shard_rank;        /* this ctx renders rows y with y % shard_count == shard_rank        */
    uint32_t shard_count;       /* 1 = whole image                                                   */
    uint32_t frames_in_flight;  /* frames traced concurrently per wavefront pass; 0 = auto           */
} spt_config;

/* Counters since the last spt_stats_clear. Per-kernel times are only collected while profiling
 * events are enabled (spt_set_profiling, SPT_PROFILE_EVENTS); they are HIP-event times on the ctx
 * stream. segments / radiance_updates / lane_* of the persistent schedules (k_paths, k_frame; their
 * time and launches are persistent_ms / persistent_launches) are only counted with
 * SPT_PROFILE_COUNTERS (the wavefront schedules count them always: their queues need the lengths). */
#define SPT_MAX_BOUNCES 32
typedef struct spt_stats {
    uint64_t frames;                          /* frames accumulated                          */
    uint64_t paths;                           /* camera paths traced (= samples)             */
    uint64_t segments[SPT_MAX_BOUNCES];       /* rays traced at each bounce depth            */
    uint64_t segments_total;
    uint64_t passes;                          /* wavefront passes launched                   */
    /* profiling (0 when disabled) */
    uint64_t extend_launches;                 /* k_extend launches timed                     */
    double extend_ms;                         /* summed k_extend duration                    */
    uint64_t extend_segments;                 /* rays processed by the timed k_extend launches */
    uint64_t shade_launches;
    double shade_ms;
    double other_ms;                          /* generate + accumulate                       */
    double extend_ms_bounce[SPT_MAX_BOUNCES]; /* k_extend time per bounce depth              */
    double shade_ms_bounce[SPT_MAX_BOUNCES];  /* k_shade time per bounce depth               */
    uint64_t bvh_nodes;                       /* nodes in the uploaded BVH (0 = flat scene)  */
    uint64_t scene_bytes;                     /* device bytes of node + primitive arrays     */
    uint64_t radiance_updates[SPT_MAX_BOUNCES]; /* per bounce >= 1: misses/emitter hits that
                                                   read-modify-wrote a path's radiance          */
    double tail_ms;                           /* k_trace_tail time (profiling)                */
    uint64_t tail_launches;
    uint64_t tail_bounce;                     /* bounces >= this run in k_trace_tail          */
    uint64_t fused;                           /* 1: extend+shade fused per bounce (shade_ms)  */
    double persistent_ms;                     /* k_paths time (profiling). A split launch
                                                 (view_split) counts as one launch, timed from the
                                                 earlier of its halves' starts to the later of their
                                                 ends; consecutive split launches overlap, so the sum
                                                 over launches may exceed the wall time            */
    uint64_t persistent_launches;
    uint64_t schedule;                        /* SPT_SCHEDULE_* the last spt_render used      */
    uint64_t lane_slots;                      /* k_paths: 64 x wave tracing steps              */
    uint64_t lane_busy;                       /* k_paths: lanes that traced a segment in them  */
    uint64_t bvh_node_visits;                 /* k_paths, BVH scenes: interior nodes visited   */
    uint64_t prim_tests;                      /* k_paths, BVH scenes: primitives tested        */
    uint64_t flat_fast_path;                  /* 1: the scene is in the range of the flat loop's
                                                 unscaled-division fast path (same results)     */
    uint64_t specialized;                     /* 1: the last k_paths / k_frame launch ran the kernel
                                                 compiled for the flat scene's shape (same results) */
    uint64_t shadow_rays;                     /* SPT_FLAG_NEE: shadow rays traced by k_paths / k_frame
                                                 (counted with SPT_PROFILE_COUNTERS)              */
    uint64_t emitters;                        /* emitters SPT_FLAG_NEE samples in the current scene */
    uint64_t stack_bytes;                     /* BVH scenes: device bytes of the persistent kernels'
                                                 traversal stacks (not in scene_bytes)            */
    uint64_t stack_need;                      /* BVH scenes: the most entries a traversal stack of the
                                                 tree holds; spt_set_scene refuses a tree needing
                                                 more than 96 (SPT_ERR_CAPACITY)                   */
    uint64_t stalled_waves;                   /* k_paths waves that stopped at their step loop's safety
                                                 bound (a logic error; spt_get_stats then fails with
                                                 SPT_ERR_HIP after filling *out)                   */
    uint64_t view_cached;                     /* 1: the last k_paths launch ran over the view's cached
                                                 bounce 0 (spt_tuning.view_cache; same results)    */
    uint64_t view_live_pixels;                /* live pixels of the cached view (a camera hit whose
                                                 path goes on); 0 while no view is cached          */
    uint64_t flat_pairs;                      /* opposite wall pairs in the shape key of the specialized
                                                 kernel that ran last (its closest hit tests one wall of
                                                 each); 0 for the generic kernels                  */
    uint64_t flat_pair_second_passes;         /* wave-level second passes of the paired wall test (some
                                                 lane's ray starts outside the pair's slab: both walls
                                                 tested); counted by k_paths' counting forms only  */
    uint64_t view_split;                      /* 1: the last k_paths launch ran as two launches over the
                                                 two halves of the cached view, on two streams
                                                 (spt_tuning.split_streams; same results)          */
    uint64_t flat_sphere_second_passes;       /* wave-level second passes of the one-pass sphere test of
                                                 a shape with two to four spheres (some lane's ray has
                                                 two or more candidate spheres: a second root stage);
                                                 counted by k_paths' counting forms only           */
} spt_stats;

typedef struct spt_ctx spt_ctx;

/* ---- library / device ---------------------------------------------------------------------- */
int spt_abi_version(void);
/* Number of HIP devices visible (0 when the runtime has none). */
int spt_device_count(int* count);

/* ---- lifecycle (CPUPathTracer ctor/dtor, CPUPathTracer.cpp:25-41) -------------------------- */
int spt_create(spt_ctx** out, int device_id);
void spt_destroy(spt_ctx* ctx);
const char* spt_last_error(const spt_ctx* ctx);
/* Launch on a caller-owned hipStream_t (e.g. torch.cuda.current_stream().cuda_stream);
 * NULL restores the ctx's own stream. */
int spt_set_stream(spt_ctx* ctx, void* hip_stream);

/* ---- scene (rebuild_scene, CPUPathTracer.cpp:328-404) ------------------------------------- */
/* Copies the primitives, builds the acceleration structure on the host (flat list for small
 * scenes, SAH BVH otherwise), uploads it, and resets accumulation (frameCount = 0, :122-131). */
int spt_set_scene(spt_ctx* ctx, const spt_prim* prims, uint32_t n_prims,
                  const spt_material* mats, uint32_t n_mats, const spt_env* env);

/* Incremental edit (the reference re-runs rebuild_scene on any change,
 * CPUPathTracer.cpp:119-161, 328-404): replace primitives indices[0..n) of the current scene with
 * prims[0..n) (indices into the array spt_set_scene was given; materials index its material array).
 * A BVH scene keeps its tree: the changed records are uploaded in place, the bounds refitted bottom-up
 * and the node array re-uploaded — no rebuild; a flat scene re-uploads its few records. Results are
 * those of spt_set_scene with the edited array (the traversal is exact for any valid tree). Resets
 * the progressive accumulation like spt_set_scene. */
int spt_update_prims(spt_ctx* ctx, const uint32_t* indices, const spt_prim* prims, uint32_t n);

/* ---- settings / progressive state (invalidate, CPUPathTracer.cpp:119-161) ----------------- */
/* (Re)allocates device buffers when the size or shard changes, and always resets accumulation. */
int spt_configure(spt_ctx* ctx, const spt_config* cfg);
/* Zero the accumulation buffer and the frame counter (:151-154). */
int spt_reset(spt_ctx* ctx);
int spt_get_frame_count(const spt_ctx* ctx, uint32_t* frame_count);

/* ---- the hot path (render, CPUPathTracer.cpp:43-85) ---------------------------------------- */
/* Traces frames [first_frame, first_frame + n_frames): frame k is seeded with k + 1 exactly as
 * get_rng_state(.., m_frameCount + 1) (:61, :192-195), and adds each frame's radiance to the
 * accumulation buffer in frame order (:77-80). Asynchronous on the ctx stream, with one exception:
 * the first one-frame call after spt_set_scene / spt_update_prims / spt_configure / spt_set_camera /
 * spt_set_material_models stores the pixels' camera hits and, for scenes that use the compacted
 * live-pixel lists, waits for that frame to read the live-pixel count back (once per change). A camera
 * with SPT_CAMERA_JITTER has no such cache (its camera segments differ from frame to frame) and never
 * waits; nor has a scene with a METAL or DIELECTRIC material. The progressive renderer calls
 * spt_render(ctx, frame_count, 1) once per App frame. */
int spt_render(spt_ctx* ctx, uint32_t first_frame, uint32_t n_frames);
int spt_synchronize(spt_ctx* ctx);

/* ---- results (get_render_result, CPUPathTracer.cpp:87-117) ------------------------------- */
/* Number of pixels this ctx owns (width*height for shard_count 1). */
int spt_shard_pixels(const spt_ctx* ctx, uint64_t* n_pixels);
/* Copy the shard's float RGBA accumulation (n_pixels * 4 floats, row-major over the shard's rows). */
int spt_read_accum(spt_ctx* ctx, float* host_rgba);
/* Device pointer / byte size of the accumulation buffer (valid until the next spt_configure). Work the
 * caller enqueues on the ctx's stream may read it between renders: from this call until the next
 * spt_configure every split launch (spt_tuning.split_streams) waits for the ctx's stream first. */
int spt_accum_device_ptr(spt_ctx* ctx, void** dptr, size_t* bytes);
/* Stream-ordered device-to-device copy of the accumulation buffer (n_pixels * 16 bytes) to `dst`,
 * e.g. into a caller-owned tensor that a collective then gathers. */
int spt_copy_accum_device(spt_ctx* ctx, void* dst);
/* Resolve on the device: c = accum / frame_count, clamp [0,1], (uint8)(c*255) truncation,
 * r<<24 | g<<16 | b<<8 | a (Color.h:7-10), then copy n_pixels u32 to the host. */
int spt_resolve_rgba8(spt_ctx* ctx, uint32_t frame_count, uint32_t* host_out);
/* The same with RenderSettings::getExposure (Types.h:56,66) applied as the reference's commented-out
 * code would (CPUPathTracer.cpp:101-104): c = (accum / frame_count) * exposure on r, g, b (not a),
 * before the clamp. exposure = 1 is exactly spt_resolve_rgba8. */
int spt_resolve_rgba8_exposure(spt_ctx* ctx, uint32_t frame_count, float exposure, uint32_t* host_out);
/* Register the caller's host image buffer [host_out, host_out + bytes) for the two resolves above:
 * the buffer is page-locked and mapped into the GPU's address space, and a resolve into exactly
 * `host_out` (while bytes >= 4 * n_pixels) has the resolve kernel store the pixels straight into it
 * over PCIe — no device staging buffer, no DMA copy — then waits as before. Any other pointer takes
 * the staging-and-copy path. The caller keeps the memory allocated until it registers another
 * buffer, passes (NULL, 0) to unregister, or destroys the ctx (the backend's RenderResult buffer:
 * HIPPathTracer re-registers it whenever it resizes). One buffer per ctx. */
int spt_register_host_output(spt_ctx* ctx, void* host_out, size_t bytes);
/* spt_render(first_frame, n_frames) followed by spt_resolve_rgba8_exposure(frame_count, exposure,
 * host_out), with the resolve fused into the call's last frame when that frame runs the one-frame
 * kernel and host_out is the registered buffer: each pixel's RGBA8 is stored over PCIe as its path
 * ends, so the image's transfer overlaps the frame (the App's render() + get_render_result(),
 * App.cpp:230-240). frame_count is the divisor: the frames accumulated after this call. Same pixels
 * as the two calls; waits for the stream. */
int spt_render_resolve_rgba8(spt_ctx* ctx, uint32_t first_frame, uint32_t n_frames, uint32_t frame_count,
                             float exposure, uint32_t* host_out);
/* Multi-GPU assembly on the root: `gathered` (device) holds shard_count row-shards, each padded to
 * ceil(height/shard_count)*width RGBA pixels, in rank order (the layout of an all-gather /
 * gather into one tensor). Writes the full width*height RGBA image to `out` (device). */
int spt_assemble_rows(spt_ctx* ctx, const void* gathered, void* out);

/* ---- camera (superset: the reference's camera is the pinhole hard-coded in CPUPathTracer.cpp:53-73,
 * at the origin, looking down +z, 90 degrees of vertical field of view, rays through the pixels'
 * corners; its Camera.h is dead code) -------------------------------------------------------------
 * A camera is an origin and three vectors: u, the image plane's right, and v, its up, both scaled by
 * tan(vfov / 2), and w, forward. The ray of pixel (x, y) — y the full-image row — with jitter (jx, jy),
 * all in fp32 without contraction, inv_w = 1.0f / W, inv_h = 1.0f / H, aspect = (float)W / (float)H:
 *   px = (float)x + jx;  py = (float)y + jy;  u_ = px * inv_w;  v_ = 1.0f - py * inv_h;
 *   sx = (u_ * 2.0f - 1.0f) * aspect;  sy = v_ * 2.0f - 1.0f;
 *   p.c = (sx * u.c + sy * v.c) + w.c;  len = sqrtf((p.x*p.x + p.y*p.y) + p.z*p.z);  d.c = p.c / len
 * from `origin`. Without SPT_CAMERA_JITTER jx = jy = 0 (the pixel's corner, as the reference). With it
 * every path draws jx = random_float(rng), jy = random_float(rng) first, from the state the reference
 * seeds it with (get_rng_state(x, y, W, frame + 1)), and trace_ray continues with that state: the ray
 * goes through a uniform point of the pixel [x, x+1] x [y, y+1], which anti-aliases the image.
 * u = (1,0,0), v = (0,1,0), w = (0,0,1) at the origin is the reference's camera. */
#define SPT_CAMERA_JITTER 1u
typedef struct spt_camera {
    float origin[3], u[3], v[3], w[3];   /* w = forward                          */
    uint32_t flags;                      /* SPT_CAMERA_JITTER                    */
    uint32_t reserved[3];                /* must be 0                            */
} spt_camera;
/* Set the camera of later spt_render calls (copied); NULL restores the reference's camera, bit for bit
 * what a ctx that never had one renders. SPT_ERR_INVALID for a non-finite value, a zero w, an unknown
 * flag or a non-zero reserved word. Resets the progressive accumulation like spt_set_env_map, and the
 * one-frame kernel's camera-hit cache. Valid before or after spt_configure; kept across spt_configure.
 * The origin may lie anywhere: a BVH scene's boxes are padded for the larger of the scene's coordinate
 * magnitude and the origin's, so a camera outside the scene's magnitude makes this call refit
 * the tree and upload its nodes again (as does the next camera back inside); closest hits equal testing every
 * primitive, which tests/test_gpu_bvh_brute.py checks up to an origin 1000 scene magnitudes away. At such
 * distances the fp32 primitive tests themselves are coarse (a sphere's reports hits within 1e-3 of the
 * distance): the image is what those tests give, on every schedule. */
int spt_set_camera(spt_ctx* ctx, const spt_camera* camera);
/* Host only: the camera at `eye` looking at `target`, computed in double and rounded once:
 * f = normalize(target - eye), r = normalize(cross(up, f)), t = cross(f, r), h = tan(vfov / 2);
 * u = r * h, v = t * h, w = f, flags 0. SPT_ERR_INVALID for eye == target, up parallel to the view
 * direction, or vfov_degrees outside (0, 180). */
int spt_camera_look_at(const float eye[3], const float target[3], const float up[3], float vfov_degrees,
                       spt_camera* out);
/* Host only: the ray (o, d) of pixel (x, y) of a width x height image with jitter (jx, jy), by the
 * function the kernels compile (csrc/spt_device.h camera_ray_dir): the same bits. */
int spt_camera_ray(const spt_camera* camera, uint32_t width, uint32_t height, uint32_t x, uint32_t y,
                   float jx, float jy, float o[3], float d[3]);

/* ---- thin lens (superset: depth of field) -----------------------------------------------------------
 * A lens belongs to the ctx's camera: an aperture of `radius` (world units) and a `focus_distance` f.
 * In focus is the plane of the points origin + f * p, p the un-normalized image-plane vector above (for a
 * spt_camera_look_at camera, |w| = 1: the plane at distance f in front of the eye). The ctx derives, in
 * double and rounded once,  a = (float)(radius / |u|),  b = (float)(radius / |v|)  (|u| = sqrt((u.x*u.x +
 * u.y*u.y) + u.z*u.z); 0 for a zero vector). A path's ray, in fp32 without contraction, with correctly
 * rounded sqrtf and '/', px ... p as above (jx = jy = 0 or the two jitter draws first):
 *   u1 = random_float(rng);  u2 = random_float(rng);
 *   r = sqrtf(u1);  phi = 2.0f * pi_f * u2;  (sp, cp) = the integrator's fp64 sin and cos of (double)phi;
 *   lx = (float)((double)r * cp);  ly = (float)((double)r * sp);  ax = lx * a;  ay = ly * b;
 *   off.c = ax * u.c + ay * v.c;   o.c = origin.c + off.c;   t.c = f * p.c - off.c;
 *   len = sqrtf((t.x*t.x + t.y*t.y) + t.z*t.z);  d.c = t.c / len
 * and trace_ray continues with the RNG state after these draws: per path the jitter's two draws (if set),
 * the lens's two, then everything as without a lens. Every schedule gives the same bits. A lens camera
 * renders as a jittered one does (a camera ray per path: no camera-hit cache, no view cache). The
 * first-hit features stay the chief ray's — the same camera's without a lens. */
typedef struct spt_lens {   /* 16 bytes */
    float radius;           /* the aperture's, world units; finite, >= 0; 0: no lens */
    float focus_distance;   /* finite, > 0 */
    uint32_t reserved[2];   /* must be 0 */
} spt_lens;
/* Set the lens of the ctx's camera (copied); NULL or radius == 0 removes it, bit for bit what the ctx
 * rendered before it had one. SPT_ERR_INVALID without a camera (spt_set_camera first: the reference's
 * pinhole has no lens), for a non-finite or negative radius, a non-finite or non-positive
 * focus_distance, or a non-zero reserved word. Resets the progressive accumulation and the caches of the
 * camera's rays as spt_set_camera does; the feature images stay valid. spt_set_camera(ctx, camera) keeps
 * the lens (a and b follow the new u and v), spt_set_camera(ctx, NULL) drops it; kept across spt_configure. */
int spt_set_camera_lens(spt_ctx* ctx, const spt_lens* lens);
/* Host only: the lens ray (o, d) of pixel (x, y) with jitter (jx, jy) and aperture sample (u1, u2), by
 * the function the kernels compile (csrc/spt_device.h camera_lens_ray): the same bits. u1 and u2 are
 * random_float values, in [0, 1] (the sine and cosine are stated for phi in [0, 2 pi] only);
 * SPT_ERR_INVALID outside that, NaN included, and for an invalid lens. */
int spt_camera_lens_ray(const spt_camera* camera, const spt_lens* lens, uint32_t width, uint32_t height,
                        uint32_t x, uint32_t y, float jx, float jy, float u1, float u2, float o[3], float d[3]);
/* Host only: the focus distance that puts the point at distance t along the camera ray of pixel (x, y)
 * with jitter (jx, jy) in focus: (float)(t / |p|), p in double from the camera's float fields.
 * SPT_ERR_INVALID for a non-finite t or t <= 0. With spt_read_features' feat_b.w as t: click to focus. */
int spt_camera_focus_at_hit(const spt_camera* camera, uint32_t width, uint32_t height, uint32_t x, uint32_t y,
                            float jx, float jy, float t, float* focus_distance);

/* ---- materials (superset, north_star "BRDF + light sampling": the reference shades one Lambertian
 * surface of albedo 0.7, CPUPathTracer.cpp:260-274) -----------------------------------------------
 * Each material of the scene has a model beside its albedo and emission: DIFFUSE (the reference's
 * cosine-weighted bounce, the default), METAL (a mirror, roughened by `fuzz`) or DIELECTRIC (glass of
 * index of refraction `ior`). At a hit everything up to and including T *= albedo (the albedo tints
 * metal and glass) and Russian roulette is as before. Then, all in fp32 without contraction, with
 * correctly rounded sqrtf and '/', dot(a,b) = (a.x*b.x + a.y*b.y) + a.z*b.z and normalize(v) =
 * v * (1.0f / sqrtf(dot(v,v))):
 *   d: the incoming direction;  n: the shading normal (a sphere's points outward, a quad's or
 *   triangle's faces the ray);  entering: a sphere: not (dot(d,n) > 0); a quad or triangle: hit on the
 *   side of its stored normal cross(u,v) / cross(v1-v0, v2-v0) (a closed mesh wound outward is a
 *   solid);  nf = -n for a sphere that is not entering, n otherwise.
 *   DIFFUSE: as the reference: direction get_random_bounche(n), origin hit + n*1e-4 (inside a sphere
 *     too: n stays the outward normal there).
 *   METAL(f): c = dot(d,nf);  r.k = d.k - (2.0f*c)*nf.k;  if f > 0: b = get_random_bounche(nf) (two
 *     draws), r.k = r.k + f*b.k;  r = normalize(r);  if not dot(r,nf) > 0 the path ends (absorbed, it
 *     adds nothing more);  otherwise origin hit + nf*1e-4. f == 0 draws nothing.
 *   DIELECTRIC(ior): always one draw u = random_float();  eta = entering ? 1.0f/ior : ior;
 *     ci = fminf(-dot(d,nf), 1.0f);  s2 = fmaxf(1.0f - ci*ci, 0.0f);  k = (eta*eta)*s2;
 *     ct = sqrtf(fmaxf(1.0f - k, 0.0f));  q = (1.0f - ior)/(1.0f + ior);  r0 = q*q;
 *     x = 1.0f - (entering ? ci : ct);  x2 = x*x;  R = r0 + (1.0f - r0)*((x2*x2)*x);
 *     if k > 1.0f || R > u: reflect exactly as METAL(0) around nf (normalized, absorbed unless
 *     dot(r,nf) > 0);  otherwise t.k = eta*(d.k + ci*nf.k) - ct*nf.k, normalized, origin
 *     hit - nf*1e-4 (transmitted). The throughput is not rescaled.
 * RNG draw order per hit: the NEE light sample (3 draws) only at a DIFFUSE hit, then Russian roulette,
 * then the model's draws. With SPT_FLAG_NEE a METAL or DIELECTRIC hit draws no light sample and traces
 * no shadow ray, and a hit's emission counts iff it is on the camera segment or the previous vertex was
 * METAL or DIELECTRIC (so an emitter seen in a mirror counts exactly once). Every schedule gives the
 * same bits. */
typedef enum spt_material_kind { SPT_MAT_DIFFUSE = 0, SPT_MAT_METAL = 1, SPT_MAT_DIELECTRIC = 2 } spt_material_kind;
typedef struct spt_material_model {   /* 16 bytes */
    uint32_t kind;        /* spt_material_kind */
    float    param;       /* METAL: fuzz in [0,1]; DIELECTRIC: index of refraction, finite, > 0 (1 is allowed);
                             DIFFUSE: must be 0 */
    uint32_t reserved[2]; /* must be 0 */
} spt_material_model;
/* One model per material of the current scene, in the order of spt_set_scene's material array; n must
 * equal that array's length. NULL (n ignored) restores all-diffuse, bit for bit what a ctx that never
 * called this renders (an array of DIFFUSE models too: both run the kernels without any material code).
 * spt_set_scene resets to all-diffuse; spt_update_prims keeps the models (they belong to materials, not
 * to primitives). Resets the progressive accumulation and the one-frame kernel's camera-hit cache, like
 * spt_set_camera. SPT_ERR_NO_SCENE before a scene; SPT_ERR_INVALID for an unknown kind, a parameter out
 * of range or non-finite, a non-zero reserved word, or a wrong n. */
int spt_set_material_models(spt_ctx* ctx, const spt_material_model* models, uint32_t n);
/* Host only: the scattering step the kernels compile (csrc/spt_device.h bsdf_scatter), the same bits.
 * d: the incoming direction; n: the surface's unit normal on its outside, so nf = entering ? n : -n (a
 * sphere's shading normal; for a quad or triangle hit from behind, the negated shading normal); *rng:
 * the path's RNG state, advanced by the model's draws. DIFFUSE returns get_random_bounche(n) around n as
 * given. dir_out: the new direction; *transmitted: it leaves on the far side (origin hit - nf*1e-4);
 * *absorbed: the path ends (dir_out is then the rejected direction). SPT_ERR_INVALID for a null pointer
 * or an invalid model. */
int spt_bsdf_sample(const spt_material_model* model, const float d[3], const float n[3], int entering,
                    uint32_t flags, uint32_t* rng, float dir_out[3], int* transmitted, int* absorbed);

/* ---- first-hit features and the denoiser (superset: the reference shows the noisy mean) -------------
 * spt_render_features traces one camera ray per shard pixel — the reference's pinhole without a camera,
 * the posed camera's ray through the pixel's corner (jx = jy = 0), through (0.5f, 0.5f) with
 * SPT_CAMERA_JITTER: the bits spt_camera_ray gives; no RNG draw — finds its closest hit as spt_render
 * does (smallest t >= 0.001, ties to the lowest index) and writes three float4 images, laid out and
 * row-sharded as the accumulation buffer:
 *   feat_a = (P.x, P.y, P.z, bits(material)),  P.c = o.c + t*d.c        miss: (0, 0, 0, bits 0xFFFFFFFF)
 *   feat_b = (n.x, n.y, n.z, t)                                          miss: (0, 0, 0, +inf)
 *   albedo = (albedo.r, albedo.g, albedo.b, bits(primitive))             miss: (0, 0, 0, bits 0xFFFFFFFF)
 * material: spt_prim.material; primitive: the index into spt_set_scene's array; n: the shading normal,
 * ng * (1.0f / sqrtf((ng.x*ng.x + ng.y*ng.y) + ng.z*ng.z)) with ng = P - centre for a sphere (outward,
 * never flipped) and the stored normal of a quad or triangle flipped to face the ray. Material models do
 * not change the images (a mirror reports its own surface). The buffers are allocated by the first call
 * and kept until spt_set_scene, spt_update_prims, spt_configure or spt_set_camera invalidates them.
 * Asynchronous on the ctx stream; touches neither the accumulation, the frame count, the one-frame
 * kernel's camera-hit cache nor any spt_stats field. SPT_ERR_NO_SCENE / SPT_ERR_NOT_CONFIGURED as spt_render. */
int spt_render_features(spt_ctx* ctx);
/* Copy the shard's feature images to the host (n_pixels * 4 floats each; any pointer may be NULL),
 * rendering them first if they are stale. Waits for the stream. */
int spt_read_features(spt_ctx* ctx, float* feat_a, float* feat_b, float* albedo);
/* Device pointers of the three images (any out pointer may be NULL) and the byte size of each, rendering
 * them first if they are stale; valid until the next call that invalidates them. */
int spt_features_device_ptr(spt_ctx* ctx, void** feat_a, void** feat_b, void** albedo, size_t* bytes);

/* The denoiser: an edge-avoiding a-trous wavelet filter of the mean colour c = accum / (float)frame_count
 * (all four channels), guided by feat_a and feat_b. `levels` passes; the first reads c, the others the
 * pass before. Level l has step s = 1 << l, inv_c = 1.0f / (sigma_color * 2^-l) and
 * inv_z = 1.0f / (sigma_plane * (float)s). All in fp32 without contraction, every '/' correctly rounded:
 *   lum(v) = L / (1.0f + L),  L = (0.2126f*v.r + 0.7152f*v.g) + 0.0722f*v.b   (compressed: a firefly at
 *   any value is an outlier);  dot(a,b) = (a.x*b.x + a.y*b.y) + a.z*b.z;  H = {1/16, 1/4, 3/8, 1/4, 1/16}.
 * A pixel p whose camera ray missed keeps c_p. A pixel that hit visits its 25 taps q = p + (dx, dy),
 * j = 0..4 outer with dy = (j-2)*s, i = 0..4 inner with dx = (i-2)*s:
 *   k  = H[j] * H[i]
 *   dl = (lum(c_q) - lum(c_p)) * inv_c;  r = 1.0f / (1.0f + dl*dl);  wc = k * (r*r)
 *   dn = fmaxf(dot(N_p, N_q), 0.0f), then dn = dn*dn normal_power_log2 times
 *   e  = P_q - P_p;  pd = dot(N_p, e) * inv_z;  rz = 1.0f / (1.0f + pd*pd);  geo = dn * (rz*rz)
 *   w  = wc * geo, and w = 0 unless q is inside the image and has p's material (a miss has none)
 *   sum.c += w * c_q.c (c = r, g, b: multiply, then add);  sum_w += w
 * and out.rgb = sum.rgb / sum_w, out.a = c_p.a (the centre tap has w > 0). */
typedef struct spt_denoise_params {   /* 32 bytes */
    uint32_t levels;             /* 1..6; default 5                                     */
    float    sigma_color;        /* > 0, finite; default 1.0f                           */
    float    sigma_plane;        /* > 0, finite, world units; default 0.05f             */
    uint32_t normal_power_log2;  /* 0..7; default 5 (the normals' cosine to the 32nd)   */
    uint32_t reserved[4];        /* must be 0                                           */
} spt_denoise_params;
/* Host only: the defaults above. SPT_ERR_INVALID for NULL. */
int spt_denoise_params_default(spt_denoise_params* out);
/* Filter the frames accumulated so far (frame_count: the divisor) into the ctx's denoised image; the
 * features are rendered first if they are stale. params = NULL: the defaults. Asynchronous on the ctx
 * stream; the accumulation, the frame count and the stats are untouched. SPT_ERR_NO_SCENE /
 * SPT_ERR_NOT_CONFIGURED as spt_render; SPT_ERR_INVALID for frame_count == 0, a parameter out of range,
 * a non-zero reserved word, or a ctx that renders a row shard (shard_count != 1: the filter needs the
 * whole image). */
int spt_denoise(spt_ctx* ctx, uint32_t frame_count, const spt_denoise_params* params);
/* Measurement and tests (the image never depends on it): the kernel form of every level of later
 * spt_denoise calls: 0 one thread per pixel with 25 global taps, 1 a residue class's tile staged in LDS,
 * -1 (the default) whichever measured faster at each step. SPT_ERR_INVALID otherwise. It
 * governs the levels of spt_denoise_guided in the same way (their own table per step). */
int spt_set_denoise_form(spt_ctx* ctx, int form);
/* The last spt_denoise's image: copied to the host (n_pixels * 4 floats; waits for the stream), or its
 * device pointer and byte size (valid until the next spt_denoise or spt_configure). SPT_ERR_INVALID
 * before any spt_denoise since the last spt_configure. */
int spt_read_denoised(spt_ctx* ctx, float* host_rgba);
int spt_denoised_device_ptr(spt_ctx* ctx, void** dptr, size_t* bytes);
/* spt_resolve_rgba8_exposure of the denoised image (it is a mean: divisor 1), into the registered host
 * buffer directly when host_out is that buffer, through the staging copy otherwise; waits for the stream.
 * SPT_ERR_INVALID before any spt_denoise. */
int spt_resolve_denoised_rgba8(spt_ctx* ctx, float exposure, uint32_t* host_out);
/* Host only, no device needed: the filter above on the caller's arrays by the function the kernels
 * compile (csrc/spt_atrous.h atrous_pixel): the same bits as spt_denoise. rgba: the mean colour,
 * feat_a / feat_b: the features, out: the result; width * height * 4 floats each (out may be rgba).
 * params = NULL: the defaults. SPT_ERR_INVALID for a null array, a zero size or an invalid parameter. */
int spt_atrous_host(const float* rgba, const float* feat_a, const float* feat_b, uint32_t width, uint32_t height,
                    const spt_denoise_params* params, float* out);

/* ---- variance-guided denoiser (superset) -------------------------------------------------------------
 * The filter above smooths a converged pixel as hard as a noisy one: its colour weight has a fixed width. This
 * one takes the width from the noise estimate's moments (below, "noise estimate"): a pixel's colour weight
 * narrows as the variance of its mean luminance falls, so the image sharpens as frames accumulate. Each level
 * also propagates the variance of what it wrote, which the next level reads.
 *
 * Definition (spt_atrous_guided_host computes it on the CPU from the functions the kernels compile,
 * csrc/spt_atrous_guided.h: the same bits). Everything is fp32 without contraction, every '/' correctly
 * rounded; only + - * / and fmaxf are used.
 *
 * Inputs: the mean colour c = accum / (float)frame_count on all four channels, as spt_denoise takes it; the
 * ctx's noise moments, a float4 (mean, m2, prevL, 0) per pixel; the host's batch count B >= 2; feat_a and feat_b.
 * Host constants, computed once:
 *   inv = 1.0f / ((float)(B - 1) * (float)frame_count);   s2 = sigma_variance * sigma_variance;
 *   per level l: step s = 1 << l, inv_z = 1.0f / (sigma_plane * (float)s).
 * Variance of the mean luminance: v0 = fmaxf(m2 * inv, 0.0f), for every pixel, hit or miss.
 * Prefilter (prefilter != 0, the default): G = {0.25f, 0.5f, 0.25f}; the 3 x 3 window's taps q = p + (i-1, j-1)
 * inside the image, rows j = 0..2 outer, columns i = 0..2 inner, both sums starting at 0.0f:
 *   g = G[j] * G[i];  s += g * v0_q;  sg += g;          then v = s / sg.     Prefilter off: v = v0.
 * Level l reads the colour c and the variance v of the pass before; the first reads the mean and the
 * (prefiltered) variance above. A pixel p whose camera ray missed keeps c_p and v_p. A pixel that hit computes
 *   iv = 1.0f / (s2 * v_p + variance_floor)
 * and visits the 25 taps in spt_denoise's order, with the same H and the same in-image rule:
 *   L(x) = (0.2126f*x.r + 0.7152f*x.g) + 0.0722f*x.b      (linear, not compressed: v is its variance)
 *   dl = L(c_q) - L(c_p);  x2 = (dl*dl) * iv;  r = 1.0f / (1.0f + x2);  wc = (H[j]*H[i]) * (r*r)
 *   dn, pd, rz and geo exactly as in spt_denoise's definition
 *   w = wc * geo, and w = 0 unless q has p's material
 *   sum.c += w * c_q.c (c = r, g, b: multiply, then add);  sw += w;  sv += (w*w) * v_q
 * and out.rgb = sum.rgb / sw, out.a = c_p.a, out_v = sv / (sw*sw). The centre tap has w = H[2]*H[2] > 0, so
 * no division by zero occurs. The width does not shrink per level: the propagated variance does that.
 * Not covered: a guided filter of the blended or reprojected image (its variance is not tracked), row shards
 * (refused as spt_denoise refuses them), per-channel variance, variance-driven adaptive sampling. */
typedef struct spt_guided_params {   /* 32 bytes */
    uint32_t levels;             /* 1..6; default 5                                                      */
    float    sigma_variance;     /* > 0, finite; default 4.0f: the colour weight's width in standard
                                    deviations of the pixel's mean luminance                             */
    float    sigma_plane;        /* > 0, finite, world units; default 0.05f                              */
    uint32_t normal_power_log2;  /* 0..7; default 5                                                      */
    float    variance_floor;     /* > 0, finite; default 1e-8f (0 would make 0 * inf a NaN)              */
    uint32_t prefilter;          /* 0 or 1; default 1                                                    */
    uint32_t reserved[2];        /* must be 0                                                            */
} spt_guided_params;
/* Host only: the defaults above. SPT_ERR_INVALID for NULL. */
int spt_guided_params_default(spt_guided_params* out);
/* Filter the frames accumulated so far (frame_count: the divisor) with the ctx's noise moments into the ctx's
 * denoised image: spt_read_denoised, spt_denoised_device_ptr, spt_resolve_denoised_rgba8 and SPT_IMAGE_DENOISED
 * serve it as they serve spt_denoise's. The features are rendered first if they are stale. params = NULL: the
 * defaults. Asynchronous on the ctx stream; the accumulation, the frame count, the stats and the moments are
 * untouched. The first call allocates two variance planes (4 bytes per pixel each) beside the filter's two
 * images; a ctx that never calls it allocates nothing for it. Errors as spt_denoise, and SPT_ERR_INVALID while
 * the ctx has folded fewer than two batches (spt_noise_update) since the accumulation last restarted. */
int spt_denoise_guided(spt_ctx* ctx, uint32_t frame_count, const spt_guided_params* params);
/* The variance the last spt_denoise_guided propagated, one float per pixel, copied to the host (waits for the
 * stream): what noise the filter left. SPT_ERR_INVALID when the current denoised image did not come from
 * spt_denoise_guided (none yet, or spt_denoise / spt_denoise_blended replaced it). */
int spt_read_denoised_variance(spt_ctx* ctx, float* host_v);
/* Host only, no device needed: the filter above on the caller's arrays by the functions the kernels compile:
 * the same bits as spt_denoise_guided. rgba: the mean colour, moments: the noise moments, feat_a / feat_b: the
 * features, out: the result; width * height * 4 floats each (out may be rgba). out_variance (may be NULL):
 * width * height floats. params = NULL: the defaults. SPT_ERR_INVALID for a null array, a zero size,
 * batches < 2, frame_count == 0 or an invalid parameter. */
int spt_atrous_guided_host(const float* rgba, const float* moments, const float* feat_a, const float* feat_b,
                           uint32_t width, uint32_t height, uint32_t batches, uint32_t frame_count,
                           const spt_guided_params* params, float* out, float* out_variance);

/* ---- temporal reprojection (superset: the reference restarts at 1 spp whenever anything changes) -------
 * After a camera move the image the old view accumulated is reused: nearly every surface is Lambertian, its
 * outgoing radiance does not depend on the eye, so what the old view gathered at a world point is an estimate
 * for the pixel that sees that point now. All arithmetic below is fp32 without contraction, '/' correctly
 * rounded; the operations are + - * /, floorf, fabsf, fminf, comparisons and one float -> int conversion of a
 * range-checked value; dot(a,b) = (a.x*b.x + a.y*b.y) + a.z*b.z.
 *
 * A captured view is an image hc (rgb: a mean radiance; a: its length n in frames, >= 1), that view's feat_a
 * and feat_b (ha, hb) and its camera. From the camera's float fields the ctx derives, in double and rounded
 * once to float, the dual basis of (u, v, w):
 *   cross(a,b) = (a.y*b.z - a.z*b.y, a.z*b.x - a.x*b.z, a.x*b.y - a.y*b.x);  c = cross(v,w);
 *   det = (u.x*c.x + u.y*c.y) + u.z*c.z;  ru = cross(v,w)/det;  rv = cross(w,u)/det;  rw = cross(u,v)/det
 * (all three rows zero if det is 0 or not finite: nothing is reused then), o' = its origin, and j' = 0.5f if it
 * had SPT_CAMERA_JITTER, else 0 (where its features' rays went). No camera: the reference's, identity rows,
 * origin 0, j' = 0.
 *
 * Reprojection of the captured view into the current one, per pixel p with the current feat_a = (P, mat),
 * feat_b = (N, t); Wf = (float)W, Hf = (float)H, aspect = Wf / Hf; "none" is out = (0, 0, 0, 0):
 *   1. mat is the miss value: none.
 *   2. mat's model is METAL or DIELECTRIC (their radiance depends on the eye): none.
 *   3. e = P - o';  a = dot(ru,e);  b = dot(rv,e);  c = dot(rw,e);  unless c > 0: none.
 *   4. sx = a / c;  sy = b / c;
 *      fx = ((sx / aspect + 1.0f) * 0.5f) * Wf - j';   fy = (1.0f - (sy + 1.0f) * 0.5f) * Hf - j';
 *      unless fx > -1.0f && fx < Wf && fy > -1.0f && fy < Hf: none (NaN and inf fall out here).
 *   5. x0f = floorf(fx);  ax = fx - x0f;  x0 = (int)x0f;  the same for y. Four taps q = (x0 + i, y0 + j),
 *      j = 0, 1 outer and i = 0, 1 inner, k = (i ? ax : 1.0f - ax) * (j ? ay : 1.0f - ay). A tap is valid iff
 *      q is inside the image, ha_q's material bits equal mat, dot(N, hb_q.xyz) >= normal_min and
 *      fabsf(dot(N, ha_q.xyz - P)) <= plane_tolerance * t. A valid tap adds
 *      sum.c += k * hc_q.c (c = r, g, b: multiply, then add);  sum_n += k * hc_q.a;  sum_w += k
 *      and any other tap nothing (its hc is not read).
 *   6. unless sum_w >= min_weight: none. Otherwise out.rgb = sum.rgb / sum_w,
 *      out.a = fminf(sum_n / sum_w, max_history).
 * The material alone does not tell surfaces apart (Cornell's floor, ceiling, back wall and spheres share one):
 * the normal and plane tests do. The primitive index is not used: it would reject every neighbouring triangle
 * of a mesh.
 *
 * Blend of the reprojected history h with the frames accumulated since: f = (float)frame_count,
 * m = accum / f on all four channels (the denoiser's mean);
 *   out.rgb = h.a > 0 ? (h.rgb * h.a + m.rgb * f) / (h.a + f) : m.rgb   (exactly those operations);  out.a = m.a
 * and out = m without an active history. A capture stores the same rgb with a = h.a + f (f without a
 * history), so lengths chain across moves and max_history caps them at the next reprojection: a camera that
 * moves every frame shows an exponential average.
 *
 * With a lens the features stay the chief ray's, as for the denoiser: reuse is then approximate (a defocused
 * pixel gathers radiance from around its chief ray's hit), not refused. Not covered: moving geometry
 * (spt_update_prims drops the history), reuse on or through metal and glass, row shards. */
typedef struct spt_reproject_params {   /* 32 bytes */
    float    max_history;      /* finite, >= 1; default 32.0f: the most frames a history counts for  */
    float    normal_min;       /* finite; default 0.9f: the least cosine between the two normals     */
    float    plane_tolerance;  /* finite, >= 0; default 0.01f: distance from the pixel's tangent
                                  plane, as a share of the pixel's hit distance t                    */
    float    min_weight;       /* finite, > 0; default 0.01f: the least sum of valid taps' weights   */
    uint32_t reserved[4];      /* must be 0                                                           */
} spt_reproject_params;
/* Host only: the defaults above. SPT_ERR_INVALID for NULL. */
int spt_reproject_params_default(spt_reproject_params* out);
/* Store what is shown now — the blend of the active history (if any) with the frame_count frames accumulated
 * (frame_count: the divisor) — as the ctx's captured view, with its length, the feature images (rendered first
 * if they are stale) and the camera. Replaces an earlier capture; the active history stays. Asynchronous on
 * the ctx stream; the buffers are allocated by the first call. SPT_ERR_NO_SCENE / SPT_ERR_NOT_CONFIGURED as
 * spt_denoise; SPT_ERR_INVALID for frame_count == 0 or a ctx that renders a row shard (shard_count != 1). */
int spt_history_capture(spt_ctx* ctx, uint32_t frame_count);
/* Map the captured view into the current one with the current camera's features (rendered first if they are
 * stale); the result becomes the ctx's active history. params = NULL: the defaults. Asynchronous on the ctx
 * stream. SPT_ERR_INVALID without a capture, for a parameter out of range or a non-zero reserved word. */
int spt_reproject(spt_ctx* ctx, const spt_reproject_params* params);
/* Drop the capture and the active history (their memory stays with the ctx until spt_configure). */
int spt_history_clear(spt_ctx* ctx);
/* The active history, rgb + length per pixel (zeros where nothing was reused): copied to the host (n_pixels * 4
 * floats; waits for the stream), or its device pointer and byte size (valid until the next spt_reproject or
 * spt_configure). SPT_ERR_INVALID without an active history. */
int spt_read_history(spt_ctx* ctx, float* host_rgba);
int spt_history_device_ptr(spt_ctx* ctx, void** dptr, size_t* bytes);
/* Write the blend of the active history with the frame_count frames accumulated (the mean alone without an
 * active history) into the ctx's blended image. Asynchronous on the ctx stream; errors as spt_history_capture. */
int spt_history_blend(spt_ctx* ctx, uint32_t frame_count);
/* The last spt_history_blend's image, as spt_read_denoised / spt_denoised_device_ptr /
 * spt_resolve_denoised_rgba8 give the denoised one (it is a mean: divisor 1; the registered host buffer is
 * written directly). SPT_ERR_INVALID before any spt_history_blend since the last spt_configure. */
int spt_read_blended(spt_ctx* ctx, float* host_rgba);
int spt_blended_device_ptr(spt_ctx* ctx, void** dptr, size_t* bytes);
int spt_resolve_blended_rgba8(spt_ctx* ctx, float exposure, uint32_t* host_out);
/* spt_denoise over the blended image instead of accum / frame_count, into the ctx's denoised image (read it with
 * spt_read_denoised / spt_resolve_denoised_rgba8). SPT_ERR_INVALID before any spt_history_blend. */
int spt_denoise_blended(spt_ctx* ctx, const spt_denoise_params* params);
/* Measurement and tests (the images never depend on it): the memory layout later spt_history_capture calls
 * store the view in: 0 three float4 images, 1 one 48-byte record per pixel (feat_a, feat_b, image), -1 (the
 * default) the one that measured faster. SPT_ERR_INVALID otherwise. */
int spt_set_history_layout(spt_ctx* ctx, int layout);
/* What drops them: spt_set_scene, spt_update_prims, spt_configure, spt_set_material_models and spt_set_env_map
 * drop the capture and the active history (the radiance changed); spt_set_camera and spt_set_camera_lens drop
 * the active history alone (the capture survives them: that is its purpose). spt_reset, spt_render, the
 * accumulation, the frame count and the stats are untouched by all of the above, and a ctx that never calls
 * them allocates nothing for them. */
/* Host only, no device needed: the captured camera as the gather reads it: rows = (ru, rv, rw), origin = o',
 * *j = j'. camera = NULL: the reference's. SPT_ERR_INVALID for a null output or an invalid camera. */
int spt_reproject_basis(const spt_camera* camera, float rows[9], float origin[3], float* j);
/* Host only, no device needed: the reprojection above on the caller's arrays by the function the kernels
 * compile (csrc/spt_reproject.h reproject_pixel): the same bits as spt_reproject. prev_camera: the captured
 * view's (NULL: the reference's); cur_a / cur_b: the current features; hist_rgba / hist_a / hist_b: the captured
 * image and features; out: the history; width * height * 4 floats each. material_reusable: one word per
 * material, 0 for a METAL or DIELECTRIC one (a material index >= n_materials counts as 0); NULL: all reusable.
 * params = NULL: the defaults. SPT_ERR_INVALID for a null array, a zero size, an invalid parameter or camera. */
int spt_reproject_host(const spt_reproject_params* params, const spt_camera* prev_camera, uint32_t width,
                       uint32_t height, const float* cur_a, const float* cur_b, const float* hist_rgba,
                       const float* hist_a, const float* hist_b, const uint32_t* material_reusable,
                       uint32_t n_materials, float* out);

/* ---- exposure and tone mapping (the reference's RenderSettings: setExposure, setAutoExposure(enabled,
 * target_luminance), getAutoExposure, getTargetLuminance) ---------------------------------------------
 * A luminance meter (an integer histogram of the image), the exposure that brings the histogram's trimmed
 * log-average to a target, and a display resolve with a tone-mapping operator. Everything the existing
 * resolves do stays as it is; these are entry points beside them. The meter caches nothing in the ctx.
 *
 * Definition (spt_display_host / spt_luminance_histogram_host compute it on the CPU from the functions the
 * kernels compile, csrc/spt_display.h: the same bits). All fp32, no contraction, `/` correctly rounded.
 *
 * Luminance and its bin, for a pixel p of an image with divisor f (the frame count for the sums, 1 for a mean):
 *   m = p / f on r, g, b;   L = (0.2126f*m.r + 0.7152f*m.g) + 0.0722f*m.b   (the denoiser's luminance)
 *   key = L > 0 ? (int)(bits(L) >> 20) : 0      (the exponent and three mantissa bits; NaN, zero, negatives: 0)
 *   bin = min(max(key, 888) - 888, 255)
 * Bin 0 is "black": everything below 2^-16 * 1.125, with NaN, zero and negatives; it is left out of the average.
 * Bins 1..254 are eight sub-bins per octave from there upward; bin 255 is everything from 2^15 * 1.875 up, +inf
 * included. Integer operations and one comparison only; the counts are uint32_t, so they do not depend on the
 * order of addition, and the counts of row shards add up to the whole image's.
 *
 * Exposure from a histogram (host only; in double, in this order, rounded to float once at the end):
 *   1. n = sum of counts[1..255]; n == 0: the exposure is 1.0f.
 *   2. lo = low_fraction * n;  hi = (1 - high_fraction) * n.
 *   3. for b = 1..255, with the cumulative count c0 before bin b and c1 = c0 + counts[b] after it:
 *        w = max(0, min(c1, hi) - max(c0, lo));  key = 888 + b;  e = (key >> 3) - 127;  k = key & 7;
 *        centre = e + log2(1 + (k + 0.5) / 8);   sw += w;  sl += w * centre.
 *   4. exposure = target_luminance / exp2(sl / sw), clamped to [min_exposure, max_exposure].
 * The two fractions are the shares of non-black pixels left out at the dark and the bright end, so that a light
 * source or a black corner does not steer the picture.
 *
 * Display transform, per channel v of r, g, b: x = (v / f) * exposure.
 *   SPT_TONEMAP_CLAMP:    clamp x to [0, 1], NaN becomes 0, (uint8)(x * 255.0f): spt_resolve_rgba8_exposure's.
 *   the other two first:  x = x > 0 ? fminf(x, 65536.0f) : 0.0f   (NaN and negatives 0; inf never reaches them)
 *   SPT_TONEMAP_REINHARD: y = x / (1.0f + x)
 *   SPT_TONEMAP_ACES:     y = (x*(2.51f*x + 0.03f)) / (x*(2.43f*x + 0.59f) + 0.14f)   (the common rational fit)
 *   both then clamp y to [0, 1] and take (uint8)(y * 255.0f).
 * Alpha is (uint8)(clamp(a / f) * 255.0f), without exposure or operator; the bytes are packed as the other
 * resolves pack them (R in the high byte). Not covered: an sRGB transfer curve, exposure smoothed over time. */
#define SPT_METER_BINS 256
enum spt_image {
    SPT_IMAGE_ACCUM = 0,     /* the accumulated sums; frame_count is the divisor                     */
    SPT_IMAGE_DENOISED = 1,  /* the last spt_denoise's image: a mean, divisor 1, frame_count ignored */
    SPT_IMAGE_BLENDED = 2    /* the last spt_history_blend's image: a mean too                       */
};
enum spt_tonemap {
    SPT_TONEMAP_CLAMP = 0,
    SPT_TONEMAP_REINHARD = 1,
    SPT_TONEMAP_ACES = 2
};
typedef struct spt_exposure_params {   /* 32 bytes */
    float    target_luminance;  /* finite, > 0; default 0.18f: RenderSettings'                          */
    float    low_fraction;      /* finite, >= 0; default 0.1f: the share of non-black pixels left out
                                   at the dark end                                                      */
    float    high_fraction;     /* finite, >= 0; default 0.02f: ... at the bright end; both below 1 in sum */
    float    min_exposure;      /* finite, > 0; default 0.015625f                                       */
    float    max_exposure;      /* finite, >= min_exposure; default 64.0f                               */
    uint32_t reserved[3];       /* must be 0                                                            */
} spt_exposure_params;
typedef struct spt_display {           /* 16 bytes */
    uint32_t tonemap;           /* spt_tonemap                                                          */
    float    exposure;          /* finite, >= 0                                                         */
    uint32_t reserved[2];       /* must be 0                                                            */
} spt_display;
/* Host only: the defaults above. SPT_ERR_INVALID for NULL. */
int spt_exposure_params_default(spt_exposure_params* out);
/* The histogram of the ctx's image (of its shard: the shards' counts add up to the whole image's) on the ctx
 * stream, waited for. SPT_ERR_NOT_CONFIGURED before spt_configure; SPT_ERR_INVALID for an unknown image, a
 * DENOISED or BLENDED image that does not exist, frame_count == 0 for ACCUM, or a null pointer. */
int spt_meter_luminance(spt_ctx* ctx, uint32_t image, uint32_t frame_count, uint32_t counts[SPT_METER_BINS]);
/* The same for n_pixels float RGBA pixels in the caller's device memory (the image spt_gather_image assembled on
 * rank 0, for one). SPT_ERR_INVALID for a null pointer, n_pixels == 0 or a divisor that is not finite and > 0. */
int spt_meter_device_image(spt_ctx* ctx, const void* device_rgba, uint64_t n_pixels, float divisor,
                           uint32_t counts[SPT_METER_BINS]);
/* The ctx's image through the display transform as RGBA8 in host_out, as spt_resolve_rgba8_exposure resolves (the
 * registered host buffer is written directly, any other through the ctx's staging image; waits). Errors as
 * spt_meter_luminance, and SPT_ERR_INVALID for an unknown operator, an exposure that is not finite and >= 0 or
 * a non-zero reserved word. */
int spt_resolve_display_rgba8(spt_ctx* ctx, uint32_t image, uint32_t frame_count, const spt_display* display,
                              uint32_t* host_out);
/* The same for the caller's device image, always through a staging image of the ctx's that grows on demand. */
int spt_resolve_display_device_image(spt_ctx* ctx, const void* device_rgba, uint64_t n_pixels, float divisor,
                                     const spt_display* display, uint32_t* host_out);
/* Measurement and tests (the counts never depend on it): the kernel form of later meterings: 0 one LDS add per
 * lane, 1 one add per distinct bin of a wave, -1 (the default) the one that measured faster.
 * SPT_ERR_INVALID otherwise. */
int spt_set_meter_form(spt_ctx* ctx, int form);
/* Host only, no device needed: the definition above by the functions the kernels compile: the same bits.
 * SPT_ERR_INVALID for a null pointer, n_pixels == 0, a divisor that is not finite and > 0, or parameters out
 * of range (a non-finite value; target_luminance, min_exposure or max_exposure not > 0; min_exposure >
 * max_exposure; a negative fraction; low_fraction + high_fraction >= 1; a non-zero reserved word). params = NULL:
 * the defaults. */
int spt_meter_bin(float luminance, uint32_t* bin);
int spt_luminance_histogram_host(const float* rgba, uint64_t n_pixels, float divisor, uint32_t counts[SPT_METER_BINS]);
int spt_exposure_from_histogram(const uint32_t counts[SPT_METER_BINS], const spt_exposure_params* params,
                                float* exposure);
int spt_display_host(const float* rgba, uint64_t n_pixels, float divisor, const spt_display* display, uint32_t* out);

/* ---- noise estimate (a superset: the reference renders until its window closes) --------------------
 * How noisy is the image, and may the renderer stop? The accumulation after a call minus the accumulation
 * before it is that call's batch of frames, and the variance of the batch means estimates the error of the
 * mean. One streaming pass beside spt_render keeps two moments of the luminance per pixel; a meter turns them
 * into a per-pixel relative error and an integer histogram of it; a host rule reads a quantile off the
 * histogram. spt_render, the accumulation, the frame count and the stats are untouched, and a ctx that never
 * calls these allocates nothing for them.
 *
 * Definition (spt_noise_update_host / spt_noise_meter_host compute it on the CPU from the functions the kernels
 * compile, csrc/spt_noise.h: the same bits). Every value is fp32 without contraction, every `/` correctly
 * rounded; only `+ - * /`, comparisons and integer operations on a float's bits are used. (Where an operation
 * creates a NaN, inf / inf or inf - inf on moments no render produces, its sign is the hardware's: the host and
 * the device then agree that e2 is a NaN, which is all its bin asks.)
 *
 * State. Per pixel one float4 (mean, m2, prevL, 0). Per ctx, on the host: the batch count B and the frames
 * folded so far W, a float holding an integer; an update that would bring W above 2^24 is refused.
 *
 * Update with a batch, the frames in (frames_before, frame_count]. Once, on the host:
 *   w = (float)(frame_count - frames_before);   Wn = W + w;   r = w / Wn.
 * Per pixel, with a the accumulation (the sums):
 *   L = (0.2126f*a.r + 0.7152f*a.g) + 0.0722f*a.b
 *   d = (L - prevL) / w;   delta = d - mean
 *   mean' = mean + r*delta;   m2' = m2 + (w*delta)*(d - mean');   prevL' = L;   the fourth word is 0.
 * Then B' = B + 1 and W' = Wn. This is West's weighted form of Welford's update: calls of different lengths
 * fold in correctly, and m2 / (B - 1) estimates the variance of one frame. The first batch after a restart
 * starts from a zeroed state with B = W = 0.
 *
 * Noise of a pixel: needs B >= 2, a pooling radius of 0..2 and a dark_floor (finite, >= 0; default 0.01f).
 *   inv = 1.0f / ((float)(B - 1) * W), once, on the host.
 *   radius 0:  s_m2 = m2;  s_mean = mean.
 *   radius > 0: each is a sum that starts at 0.0f and adds the taps of the (2*radius + 1)^2 window that lie
 *              inside the image, rows outer and columns inner, and is then divided by the tap count as a float.
 *   v = s_m2 * inv;   t = s_mean + dark_floor;   e2 = v / (t*t)
 * e2 is the squared relative standard error of the mean luminance. Its bin:
 *   bin = 255 if e2 is NaN; otherwise bin = e2 > 0 ? min(max((int)(bits(e2) >> 20), 792) - 792, 255) : 0.
 * 792 is the key of 2^-28: the bins are eight per octave from 2^-28 to 2^4, a relative error of 0.006 % to
 * 400 %. Bin 0 also holds zero, negatives and everything below; bin 255 also holds everything from 15 up,
 * +inf and NaN. The counts are uint32_t, so they do not depend on the order of addition; with radius 0 the
 * counts of row shards add up to the whole image's. Pooling is not defined on a row shard (its rows are not
 * neighbours).
 *
 * Stop rule (host, in double): total = the sum of the counts; the first bin b at which the cumulative count
 * reaches quantile * total. rel_error = sqrt(the lower edge of bin b + 1), the float whose bits are
 * (793 + b) << 20: the bin's upper edge, so it errs on the safe side. +inf for b = 255; 0 for b = 0 and for an
 * empty histogram.
 * Not covered: per-channel moments, adaptive sampling, a false-colour resolve
 * of the noise image, an estimate smoothed over time, pooling across row shards. */
#define SPT_NOISE_BINS 256
typedef struct spt_noise_params {      /* 16 bytes */
    uint32_t radius;            /* 0, 1 or 2; default 1                                                 */
    float    dark_floor;        /* finite, >= 0; default 0.01f                                          */
    uint32_t reserved[2];       /* must be 0                                                            */
} spt_noise_params;
/* Host only: the defaults above. SPT_ERR_INVALID for NULL. */
int spt_noise_params_default(spt_noise_params* out);
/* Fold the frames since the last update (or since the accumulation restarted) into the ctx's moments;
 * frame_count is the number of frames the accumulation holds, as the resolves take it. Asynchronous on the ctx
 * stream. The first call allocates the state, 16 bytes per pixel (of the shard); spt_configure frees it when it
 * reallocates the ctx's buffers. spt_reset, and with it every entry point that restarts the accumulation, sets
 * B = W = 0 and has the next update start from a zeroed state. SPT_ERR_NOT_CONFIGURED before spt_configure;
 * SPT_ERR_INVALID when frame_count is not greater than the frames already folded, or above 2^24. */
int spt_noise_update(spt_ctx* ctx, uint32_t frame_count);
/* Host only: the batches and frames folded since the last restart (either may be NULL). */
int spt_noise_batches(const spt_ctx* ctx, uint32_t* batches, uint32_t* frames);
/* The histogram of the ctx's per-pixel e2 on the ctx stream, waited for; also writes the e2 image (4 bytes per
 * pixel, allocated by the first call). params = NULL: the defaults. SPT_ERR_INVALID before the second update
 * since a restart (B < 2), for a parameter out of range or a non-zero reserved word, and for radius > 0 on a
 * row shard (shard_count > 1). */
int spt_noise_meter(spt_ctx* ctx, const spt_noise_params* params, uint32_t counts[SPT_NOISE_BINS]);
/* The state (4 floats per pixel) and the last metering's e2 image (1 float per pixel) of the shard, waited for;
 * SPT_ERR_INVALID while there is none (no update since spt_configure allocated; no metering). */
int spt_read_noise_moments(spt_ctx* ctx, float* host_moments);
int spt_read_noise(spt_ctx* ctx, float* host_e2);
/* Their device addresses, valid until the next spt_configure (either output may be NULL; an image that does not
 * exist yet gives a null address). *pixels: the shard's pixel count. */
int spt_noise_device_ptr(spt_ctx* ctx, void** moments, void** e2, uint64_t* pixels);
/* The same kernels over width * height moments in the caller's device memory, with the caller's B and W: the
 * counterpart of spt_meter_device_image, for a gathered multi-GPU image. device_e2 (may be NULL): width * height
 * floats of the caller's device memory for the per-pixel values. SPT_ERR_INVALID for a null pointer, an empty or
 * too large image (>= 2^31 pixels), batches < 2, a W that is not an integer in [1, 2^24] or invalid parameters. */
int spt_noise_meter_device_image(spt_ctx* ctx, const void* device_moments, uint32_t width, uint32_t height,
                                 uint32_t batches, float frames, const spt_noise_params* params,
                                 uint32_t counts[SPT_NOISE_BINS], void* device_e2);
/* Host only, no device needed: the definition above by the functions the kernels compile: the same bits.
 * spt_noise_update_host folds one batch of batch_frames frames into moments (n_pixels * 4 floats, in place),
 * which held frames_before frames (0: they are taken as zero, whatever they hold); accum_rgba is the accumulation
 * after the batch. SPT_ERR_INVALID for a null pointer, n_pixels == 0, a count that is not an integer, batch_frames
 * < 1 or frames_before + batch_frames > 2^24.
 * spt_noise_meter_host: counts and, if e2 is not NULL, the width * height per-pixel values; errors as
 * spt_noise_meter_device_image.
 * spt_noise_from_histogram: the stop rule; SPT_ERR_INVALID for a null pointer or a quantile outside (0, 1]. */
int spt_noise_update_host(const float* accum_rgba, uint64_t n_pixels, float batch_frames, float frames_before,
                          float* moments);
int spt_noise_meter_host(const float* moments, uint32_t width, uint32_t height, uint32_t batches, float frames,
                         const spt_noise_params* params, uint32_t counts[SPT_NOISE_BINS], float* e2);
int spt_noise_from_histogram(const uint32_t counts[SPT_NOISE_BINS], double quantile, double* rel_error);

/* ---- environment map (superset — the reference's SkyBox, Scene.h:268-278,
 * is loaded by dead code and never sampled) -------------------------------------------------- */
/* Miss radiance from an octahedral environment map instead of sample_sky's gradient (only while
 * the scene's env.sky_enabled is set): `rgba` holds width*height texels of 4 floats, texel
 * (ix, iy) at iy*width + ix; a direction d maps to the octahedron |x|+|y|+|z| = 1 (y up, lower
 * hemisphere folded over the diagonals) and takes the nearest texel (octa_texel in
 * csrc/spt_device.h). rgba = NULL restores the gradient sky. Resets the progressive accumulation. */
int spt_set_env_map(spt_ctx* ctx, const float* rgba, uint32_t width, uint32_t height);
/* Host utility: resample an equirectangular RGB image (src_width x src_height x 3 floats, row 0 at
 * +y, column 0 at phi = -pi with phi = atan2(x, -z)) into an octahedral RGBA map (dst_width x
 * dst_height x 4 floats, alpha 1), nearest source texel per destination texel centre. */
int spt_env_octa_from_equirect(const float* src_rgb, uint32_t src_width, uint32_t src_height, float* dst_rgba,
                               uint32_t dst_width, uint32_t dst_height);

/* ---- measurement --------------------------------------------------------------------------- */
enum spt_profile {
    SPT_PROFILE_EVENTS = 1,   /* HIP events around every launch (per-kernel times in spt_stats)     */
    SPT_PROFILE_COUNTERS = 2, /* k_paths counts segments per bounce (a slower kernel variant)       */
    SPT_PROFILE_SPAN = 4      /* k_paths / k_frame: ONE event pair around all their launches until
                               * profiling is switched off — from before the first launch to after
                               * the last — instead of one per launch (per-launch events cost a
                               * one-frame call ~15 %); persistent_ms is that span, persistent_launches
                               * the launches inside it. Other kernels are not timed in this mode. */
};
int spt_set_profiling(spt_ctx* ctx, int mode);  /* mode: OR of spt_profile, 0 = off */
int spt_get_stats(spt_ctx* ctx, spt_stats* out);   /* synchronizes the ctx stream */
int spt_stats_clear(spt_ctx* ctx);
/* *view_wide = 1 when the last k_paths launch ran the wide form, 64-pixel chunks over the cached view's live
 * list (spt_tuning.wide_chunks; same results), else 0. A query of its own beside spt_stats.view_cached and
 * view_split: spt_stats keeps its size. */
int spt_get_view_wide(spt_ctx* ctx, uint64_t* view_wide);
/* *flat_ranges = 1 when the last k_paths launch ran a kernel compiled with the scene's range bit in force: a flat
 * scene whose albedos are 0 or in [2^-5, 1] with one channel nonzero throughout, whose emission is >= +0, whose
 * spheres and stored normals are well scaled (DESIGN.md 3.1d states the predicate), traced with at most 9
 * bounces; the step loop then runs its divisions and inverse roots without their per-lane range tests (same
 * results). 0 for every other kernel. A query of its own, like spt_get_view_wide: spt_stats keeps its size. */
int spt_get_flat_ranges(spt_ctx* ctx, uint64_t* flat_ranges);

/* ---- multi-GPU: row shards gathered over RCCL ------------------------------
 * One process and one ctx per GPU; ctx r is configured with shard_rank = r, shard_count = N. The
 * ranks share one RCCL communicator, created from an id that rank 0 makes and the host passes to
 * the others out of band (a TCP store, MPI, a file). RCCL is resolved at run time: the copy already
 * loaded in the process (e.g. PyTorch's) is used, else librccl.so.1 from the ROCm install. */
#define SPT_COMM_ID_BYTES 128
/* SPT_OK if this process can reach RCCL (the library and the symbols spt_comm_* bind resolve; no
 * communicator and no bootstrap socket are created), SPT_ERR_NO_DEVICE otherwise. Every rank can ask
 * before the collective spt_comm_init, so that all agree on the gather path first. */
int spt_comm_available(void);
/* Rank 0: a new communicator id (ncclGetUniqueId). */
int spt_comm_unique_id(uint8_t id[SPT_COMM_ID_BYTES]);
/* Join the communicator as `rank` of `n_ranks` (ncclCommInitRank; collective: every rank calls it,
 * each on its own ctx/GPU). rank / n_ranks must equal the ctx's shard_rank / shard_count. */
int spt_comm_init(spt_ctx* ctx, const uint8_t id[SPT_COMM_ID_BYTES], int n_ranks, int rank);
/* Collective: every rank's accumulation shard, padded to ceil(height / N) rows, is gathered to rank 0
 * (one ncclGather on the ctx stream, 16 B per padded shard pixel per rank), and rank 0 de-interleaves
 * the shards into the full width*height float RGBA image at `root_image` (device memory, rank 0;
 * ignored on the others). Asynchronous on the ctx stream, like spt_render. */
int spt_gather_image(spt_ctx* ctx, void* root_image);
/* The same collective overlapped with rendering (a progressive renderer showing every step's image on
 * rank 0 while the GPUs render on): the shard is snapshot on the ctx stream (a device copy, 16 B per
 * shard pixel), and the gather and rank 0's assembly run on a stream of the ctx's own, so the next
 * spt_render calls start at once. `root_image` holds the image of the frames rendered before this
 * call once spt_gather_wait has ordered the ctx stream after it (or the device is synchronized).
 * A later gather first waits for this one to have read the snapshot. */
int spt_gather_image_overlapped(spt_ctx* ctx, void* root_image);
/* Orders the ctx stream after the last overlapped gather (no host wait); a no-op without one. */
int spt_gather_wait(spt_ctx* ctx);
/* Leave the communicator (also done by spt_destroy). */
int spt_comm_destroy(spt_ctx* ctx);

/* ---- schedule tuning (measurement and tests; results never depend on it) ----------------------
 * Every field 0 (or -1 where noted) = the library's automatic choice, which is what production uses.
 * Replaces per-process environment overrides: a tuned ctx is explicit in the caller's code. */
typedef struct spt_tuning {
    int32_t fused;             /* flat wavefront schedule: -1 auto, 0 split extend/shade, 1 fused     */
    uint32_t tail_bounce;      /* wavefront: bounces >= this run in k_trace_tail (0 auto)            */
    int32_t persistent;        /* -1 auto, 0 never k_paths, 1 k_paths for every call                  */
    int32_t frame_kernel;      /* calls of < SPT_PERSISTENT_MIN_FRAMES: -1 auto, 0 wavefront, 1 k_frame */
    uint32_t chunks_per_wave;  /* k_paths: chunks per resident wave in each small tail tier (0 = auto:
                                  4 for BVH scenes of <= 256 K primitives, 2 otherwise)                */
    uint32_t px_shift;         /* k_paths: force chunks of 1 << px_shift pixels, 2..5 (0 auto)         */
    uint32_t subqueues;        /* wavefront: block-private sub-queues (0 = 12 per CU)                  */
    uint32_t bvh_max_leaf;     /* BVH build: primitives per leaf, 1..15 (0 auto), next spt_set_scene   */
    uint32_t bvh_bins;         /* BVH build: SAH bins per axis, 2..64 (0 = 64), next spt_set_scene     */
    int32_t specialize;        /* flat scenes: the persistent kernels compiled at run time for the scene's
                                  shape (hiprtc; the generic ones if that fails). 0: compiled on a
                                  background thread started by spt_set_scene, the generic kernels run
                                  until it is ready (a render call never waits on the compiler);
                                  1: compiled inside the first launch that needs it; -1: never          */
    int32_t view_cache;        /* flat scenes, k_paths: every pixel's bounce 0 kept across the launches of a
                                  view (scene, camera, sky, size, shard and configuration unchanged) in
                                  compacted lists the launches then run over. 0: automatic, built behind
                                  the first persistent call after a change; -1: never (every launch
                                  computes bounce 0 itself)                                              */
    int32_t split_streams;     /* flat scenes, k_paths over a cached view: each launch as two, over the two
                                  halves of the view's lists, on two streams of the ctx's own, so that a
                                  launch's blocks move in while the waves of the launch before it run out of
                                  work (disjoint pixels need no order; each pixel's frames stay in stream
                                  order within its half). The ctx stream waits on both halves before
                                  spt_render returns, so work ordered behind the call sees the finished
                                  render; the halves wait on the ctx stream only after another ctx call used
                                  it, or on every call once spt_accum_device_ptr handed the sums out (the
                                  caller's own readers on the stream are then ordered before the next
                                  render's writes, as without the split). Decided once per spt_render call.
                                  0: automatic (launches of at least 2^24 live-pixel frames); 1: whenever a view is
                                  cached; -1: never                                                     */
    int32_t wide_chunks;       /* flat scenes, k_paths over a cached view: a first tier of 64-pixel chunks, every
                                  lane of a wave holding a pixel (the wide kernel; launches of at most 512
                                  frames, so a longer call runs more of them). Eligible: no NEE, no forced
                                  px_shift, a whole image (world size 1). Decided once per spt_render call.
                                  0: automatic (launches of at least 3.15 M live-pixel frames of an image
                                  whose plan already starts with 32-pixel chunks: Cornell 1080p from 4
                                  frames per call); 1: every eligible launch over a cached view; -1: never */
} spt_tuning;
/* Applies to later calls; subqueues re-sizes at the next spt_configure. */
int spt_set_tuning(spt_ctx* ctx, const spt_tuning* tuning);

/* ---- run-time specialization (flat scenes) ---------------------------------------------------
 * Flat scenes (<= 32 primitives) run k_paths / k_frame compiled for their shape — the number of
 * primitives of each kind — and the launch configuration their step loop reads (max bounces, RR
 * depth, the sky switch, SPT_FLAG_ABS_FLOAT) with hiprtc (~2 s per key and kernel, cached per process);
 * positions and materials are not baked in, so editing them re-uses the kernels. spt_set_scene and
 * spt_configure start a new key's compiles on a background thread and spt_render runs the generic
 * kernels (same results) until they are ready, so no render call stalls on the compiler.
 * spt_specialize_scene (call it after spt_configure) waits for (or runs) the current scene's
 * compiles and loads the kernels now, so the next frame runs them; a BVH scene is a no-op. */
int spt_specialize_scene(spt_ctx* ctx);
/* Host only, no device needed: compile the specialized k_paths and k_frame for the flat scene
 * `prims` (env_map: the environment-map variant; the shape alone, on run-time configuration values)
 * into the process cache. 0 on success; otherwise
 * SPT_ERR_INVALID (not a flat scene) or SPT_ERR_HIP with the compiler log in `log`. */
int spt_compile_flat_kernels(const spt_prim* prims, uint32_t n_prims, int env_map, char* log, size_t log_bytes);

/* ---- host-only scene builders (no device needed) ------------------------------------------- */
/* Capacity protocol: pass NULL arrays to query the counts, then call again with room for them.
 * Scenes are deterministic (fixed seeds). SPT_SCENE_* ids: */
typedef enum spt_scene_id {
    SPT_SCENE_C1_SPHERE_GROUND = 0, /* App.cpp:101-111: r=1 @ (0,-1,5), r=100 @ (0,-102,5)          */
    SPT_SCENE_APP_DEFAULT = 1,      /* App.cpp:98-122: the above + 6x6 grid of r=0.5 at z=10          */
    SPT_SCENE_CORNELL = 2,          /* C2/C3: 5 walls + ceiling emitter quad + 2 spheres */
    SPT_SCENE_BUNNYLIKE = 3,        /* C4: displaced icosphere (81,920 tris) in the Cornell box      */
    SPT_SCENE_INTERIOR_1M = 4       /* C5: room + 64 displaced meshes, 1,000,000 triangles            */
} spt_scene_id;
int spt_build_scene(uint32_t scene_id, spt_prim* prims, uint32_t* n_prims,
                    spt_material* mats, uint32_t* n_mats, spt_env* env);

#ifdef __cplusplus
}
#endif
#endif /* SPT_H */
