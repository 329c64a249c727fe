// Ray-level GPU checks of spt_device.h: each device function is called directly, one small kernel per
// section, on inputs built to sit on its branch points, and compared bit for bit (two NaNs equal, +inf a
// miss) with the oracle's plain C: ref_intersect, ref_bounce_dir, ref_light_sample, ref_octa_texel
// (oracle/cpu_ref.h) and mat_scatter (tests/cpp/ref_materials.c); camera_ray_dir and sincos_2pi, which
// the oracle does not state, with their own host builds (sqrtf and '/'; the same FMA sequence).
//   1 camera      camera_ray_dir: cameras on either side of every term of the device fast path's gate
//   2 intersect   isect_sphere / isect_quad / isect_tri, and isect_sphere_fast / isect_quad_axis_fast
//                 <AX, kRect> on the lanes closest_flat would send there (its per-lane gate, the scene's
//                 fast_division_ok and flat_rect_bits), with the `redo` protocol
//   3 sincos      sincos_2pi<false>, <true>; bounce_dir<false>, <true> against ref_bounce_dir
//   4 bsdf        bsdf_scatter<false>, <true> against mat_scatter
//   5 light       light_sample<true>, <false> against ref_light_sample
//   6 octa        octa_texel against ref_octa_texel
// Device records come from the product's host code (prepare_prims, sort_flat_by_kind, flat_rect_bits,
// fast_division_ok, build_emitters), so a wrong precomputed constant shows as well.
// `--host` launches nothing: it builds the same inputs, asserts that every branch they are aimed at is
// reached (the coverage counters, also asserted in a GPU run) and compares the host builds with the oracle.
// One line per section: inputs, mismatches, the first mismatching input in hex, the counters. PASS / FAIL,
// exit status 0 / 1; 2 on a HIP error (nothing is launched after one).
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "cpu_ref.h"
#include "scene.h"
#include "spt_device.h"

extern "C" int mat_scatter(const spt_material_model* m, const float d[3], const float nf[3], int entering,
                           uint32_t flags, uint32_t* rng, float out[3], int* transmitted);

using spt::F3;

namespace {

// ---- plumbing ----------------------------------------------------------------------------------------
struct HipFail {};
bool g_host = false;
double g_oracle_s = 0.0;  // time spent computing expected values

void ck(hipError_t e, const char* what) {
    if (e == hipSuccess) return;
    std::printf("HIP error: %s: %s\n", what, hipGetErrorString(e));
    throw HipFail{};
}
void ran(const char* what) {
    ck(hipGetLastError(), what);
    ck(hipDeviceSynchronize(), what);
}
template <class T>
struct Dev {
    T* p = nullptr;
    size_t n;
    explicit Dev(size_t n_) : n(n_) { ck(hipMalloc((void**)&p, (n ? n : 1) * sizeof(T)), "hipMalloc"); }
    explicit Dev(const std::vector<T>& v) : Dev(v.size()) {
        if (n) ck(hipMemcpy(p, v.data(), n * sizeof(T), hipMemcpyHostToDevice), "hipMemcpy to device");
    }
    Dev(const Dev&) = delete;
    ~Dev() { (void)hipFree(p); }
    std::vector<T> get() const {
        std::vector<T> v(n);
        if (n) ck(hipMemcpy(v.data(), p, n * sizeof(T), hipMemcpyDeviceToHost), "hipMemcpy to host");
        return v;
    }
};
inline uint32_t grid(size_t n) { return (uint32_t)((n + 255u) / 256u); }

struct Clock {
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    ~Clock() { g_oracle_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }
};

__host__ __device__ inline uint32_t hash32(uint32_t x) {
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}
inline uint32_t bits(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}
inline float fbits(uint32_t u) {
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}
// x moved by k units in the last place (through zero: -0 and +0 are one step apart)
inline float ulps(float x, int k) {
    int64_t i = bits(x);
    if (i & 0x80000000ll) i = -(i & 0x7fffffffll) - 1;
    i += k;
    return fbits(i < 0 ? (uint32_t)(-(i + 1)) | 0x80000000u : (uint32_t)i);
}
inline bool same(float a, float b) { return bits(a) == bits(b) || (a != a && b != b); }
inline bool same(double a, double b) { return std::memcmp(&a, &b, 8) == 0 || (a != a && b != b); }
inline bool same3(const float* a, const float* b) { return same(a[0], b[0]) && same(a[1], b[1]) && same(a[2], b[2]); }
// hashed floats: [0, 1), [-1, 1) and a unit vector (normalized in double, rounded once)
inline float u01(uint32_t h) { return (float)(hash32(h) >> 8) * 0x1p-24f; }
inline float s11(uint32_t h) { return u01(h) * 2.0f - 1.0f; }
inline void unit3(uint32_t h, float v[3]) {
    double x, y, z, l;
    do {
        x = s11(h * 3u + 0x1111u), y = s11(h * 3u + 0x2222u), z = s11(h * 3u + 0x3333u);
        l = std::sqrt(x * x + y * y + z * z);
        h = hash32(h + 0x9e3779b9u);
    } while (!(l > 0.05));
    v[0] = (float)(x / l), v[1] = (float)(y / l), v[2] = (float)(z / l);
}
inline float norm2(const float v[3]) { return (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]; }
// a vector with no small component whose computed (x*x + y*y) + z*z is exactly `target`
bool find_norm2(float target, uint32_t seed, float v[3]) {
    for (uint32_t tries = 0; tries < 100000u; ++tries) {
        float u[3];
        unit3(seed * 100003u + tries, u);
        if (std::fabs(u[0]) < 0.2f || std::fabs(u[1]) < 0.2f || std::fabs(u[2]) < 0.2f) continue;
        const float s = std::sqrt(target);
        for (int c = 0; c < 3; ++c) u[c] *= s;
        for (int k = -8; k <= 8; ++k) {
            v[0] = u[0], v[1] = u[1], v[2] = ulps(u[2], k);
            if (norm2(v) == target) return true;
        }
    }
    return false;
}

std::string hex(const float* f, int n) {
    std::string s;
    char b[16];
    for (int i = 0; i < n; ++i) {
        std::snprintf(b, sizeof b, "%s%08x", i ? " " : "", bits(f[i]));
        s += b;
    }
    return s;
}
std::string hexu(uint32_t u) {
    char b[16];
    std::snprintf(b, sizeof b, "%08x", u);
    return b;
}

struct Section {
    std::string name;
    uint64_t n = 0, bad = 0;
    std::string first;
    std::vector<std::pair<std::string, uint64_t>> cover;
    bool cover_ok = true;
    explicit Section(const char* nm) : name(nm) {}
    void mismatch(const std::string& what) {
        if (!bad++) first = what;
    }
    // a branch the inputs are aimed at: its count is printed, and zero fails the section
    void need(const char* what, uint64_t count) {
        cover.emplace_back(what, count);
        if (!count) cover_ok = false;
    }
    bool report() const {
        std::printf("%s: %llu inputs, %llu mismatches%s%s;", name.c_str(), (unsigned long long)n,
                    (unsigned long long)bad, bad ? ", first: " : "", first.c_str());
        for (const auto& c : cover) std::printf(" %s=%llu", c.first.c_str(), (unsigned long long)c.second);
        std::printf("%s\n", cover_ok ? "" : "  [a branch is not reached]");
        return bad == 0 && cover_ok;
    }
};

// ======================================================================================================
// 1. camera
// ======================================================================================================
__host__ __device__ inline void jitter_of(uint32_t i, uint32_t seed, float& jx, float& jy) {
    const uint32_t h = hash32(i * 2u + seed), mode = h & 3u;
    if (mode == 0u) {
        jx = jy = 0.0f;
    } else if (mode == 1u) {
        jx = jy = 0x1.fffffep-1f;  // the largest float below 1
    } else {
        jx = (float)(hash32(h) >> 8) * 0x1p-24f;
        jy = (float)(hash32(h ^ 0x9e3779b9u) >> 8) * 0x1p-24f;
    }
}

__global__ void k_camera(spt::CameraPose c, uint32_t w, uint32_t row_step, uint32_t n, float inv_w, float inv_h,
                         float aspect, uint32_t seed, F3* out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float jx, jy;
    jitter_of(i, seed, jx, jy);
    out[i] = spt::camera_ray_dir(c, i % w, (i / w) * row_step, jx, jy, inv_w, inv_h, aspect);
}

struct CamCase {
    std::string name;
    spt::CameraPose c;
};
spt::CameraPose pose(const float u[3], const float v[3], const float w[3]) {
    return spt::CameraPose{F3{0.25f, 1.0f, -2.0f}, F3{u[0], u[1], u[2]}, F3{v[0], v[1], v[2]}, F3{w[0], w[1], w[2]}};
}
spt::CameraPose scaled_identity(float su, float sv, float sw) {
    const float u[3] = {su, 0, 0}, v[3] = {0, sv, 0}, w[3] = {0, 0, sw};
    return pose(u, v, w);
}
// spt_camera_look_at's construction (double, rounded once), 90 degrees
spt::CameraPose look(double fx, double fy, double fz, double ux, double uy, double uz, double h) {
    double f[3] = {fx, fy, fz}, up[3] = {ux, uy, uz}, r[3], t[3];
    double l = std::sqrt(f[0] * f[0] + f[1] * f[1] + f[2] * f[2]);
    for (double& a : f) a /= l;
    r[0] = up[1] * f[2] - up[2] * f[1], r[1] = up[2] * f[0] - up[0] * f[2], r[2] = up[0] * f[1] - up[1] * f[0];
    l = std::sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
    for (double& a : r) a /= l;
    t[0] = f[1] * r[2] - f[2] * r[1], t[1] = f[2] * r[0] - f[0] * r[2], t[2] = f[0] * r[1] - f[1] * r[0];
    const float u[3] = {(float)(r[0] * h), (float)(r[1] * h), (float)(r[2] * h)};
    const float v[3] = {(float)(t[0] * h), (float)(t[1] * h), (float)(t[2] * h)};
    const float w[3] = {(float)f[0], (float)f[1], (float)f[2]};
    return pose(u, v, w);
}

bool check_camera() {
    Section sec("camera");
    std::vector<CamCase> cams;
    cams.push_back({"identity", scaled_identity(1, 1, 1)});
    cams.push_back({"look_at", look(0.3, -0.4, 0.8, 0.1, 1.0, 0.05, 0.7)});
    // straight down each axis: zero numerators (the general division keeps their sign)
    cams.push_back({"+x", look(1, 0, 0, 0, 1, 0, 1)});
    cams.push_back({"-x", look(-1, 0, 0, 0, 1, 0, 1)});
    cams.push_back({"+y", look(0, 1, 0, 0, 0, 1, 1)});
    cams.push_back({"-y", look(0, -1, 0, 0, 0, 1, 1)});
    cams.push_back({"+z", look(0, 0, 1, 0, 1, 0, 1)});
    cams.push_back({"-z", look(0, 0, -1, 0, 1, 0, 1)});
    cams.push_back({"u=0", scaled_identity(0, 1, 1)});
    cams.push_back({"u=v=0", scaled_identity(0, 0, 1)});
    // q = |p|^2 on either side of 2^-80 and of 2^40 (the whole camera scaled: q = s^2 (sx^2 + sy^2 + 1))
    cams.push_back({"s=2^-40", scaled_identity(0x1p-40f, 0x1p-40f, 0x1p-40f)});
    cams.push_back({"s<2^-40", scaled_identity(0x1.fffp-41f, 0x1.fffp-41f, 0x1.fffp-41f)});
    cams.push_back({"s=2^-43", scaled_identity(0x1p-43f, 0x1p-43f, 0x1p-43f)});
    cams.push_back({"s<2^20", scaled_identity(0x1.6p19f, 0x1.6p19f, 0x1.6p19f)});
    cams.push_back({"w<2^20", scaled_identity(0x1p-30f, 0x1p-30f, 0x1.fffffep19f)});
    cams.push_back({"w=2^20", scaled_identity(0x1p-30f, 0x1p-30f, 0x1p20f)});
    // numerators on either side of 2^-100 (p.x = sx * u.x) and of 2^50
    cams.push_back({"u=2^-100", scaled_identity(0x1p-100f, 1, 1)});
    cams.push_back({"u=2^-103", scaled_identity(0x1p-103f, 0x1p-101f, 1)});
    cams.push_back({"u=2^50", scaled_identity(0x1p50f, 1, 1)});
    cams.push_back({"u=2^49", scaled_identity(0x1p49f, 0x1p48f, 0x1p30f)});
    // past the gate, q in [2^40, 2^60), where the unscaled division is wrong: len = 1.5 * 2^29 and, in a
    // 2^20 x 1 image without jitter, p.x = 15 m 2^-122 for integers m: for odd m the quotient p.x / len lies
    // exactly half way between two denormals, and the unscaled sequence rounds it by the sign of its
    // reciprocal's error instead of to even
    cams.push_back({"ties", scaled_identity(0x1.ep-120f, 1, 0x1.8p29f)});
    // q next to an even power of two: sqrtf's result is decided by a residual that is exactly zero
    const float targets[4] = {0x1.fffffep-1f, 0x1.000002p0f, 0x1.fffffep1f, 0x1.000002p2f};
    uint64_t root_ties = 0;
    for (uint32_t k = 0; k < 8u; ++k) {
        float w[3];
        if (!find_norm2(targets[k & 3u], 77u + k, w)) continue;
        const float u[3] = {0x1p-60f, 0, 0}, v[3] = {0, 0x1p-60f, 0};
        cams.push_back({"q=" + hexu(bits(targets[k & 3u])), pose(u, v, w)});
        ++root_ties;
    }
    const uint32_t sizes[3][3] = {{37, 23, 1}, {1920, 1080, 7}, {1u << 20, 1, 1}};  // w, h, every n-th row

    uint64_t fast = 0, general = 0, q_lo[2] = {0, 0}, q_hi[2] = {0, 0}, n_lo[2] = {0, 0}, n_hi[2] = {0, 0};
    uint64_t zero_num = 0, oracle_bad = 0, oracle_n = 0;
    std::vector<F3> want;
    for (size_t ci = 0; ci < cams.size(); ++ci) {
        const spt::CameraPose& c = cams[ci].c;
        for (const auto& sz : sizes) {
            const uint32_t w = sz[0], h = sz[1], step = sz[2], rows = (h + step - 1u) / step, n = w * rows;
            const float inv_w = 1.0f / (float)w, inv_h = 1.0f / (float)h, aspect = (float)w / (float)h;
            const uint32_t seed = (uint32_t)ci * 977u + w;
            want.resize(n);
            {
                Clock clk;
                for (uint32_t i = 0; i < n; ++i) {
                    float jx, jy;
                    jitter_of(i, seed, jx, jy);
                    const uint32_t x = i % w, y = (i / w) * step;
                    want[i] = spt::camera_ray_dir(c, x, y, jx, jy, inv_w, inv_h, aspect);  // sqrtf and '/'
                    // the gate's terms, restated for the counters only
                    const float px = (float)x + jx, py = (float)y + jy;
                    const float sx = ((px * inv_w) * 2.0f - 1.0f) * aspect, sy = (1.0f - py * inv_h) * 2.0f - 1.0f;
                    const float p[3] = {(sx * c.u.x + sy * c.v.x) + c.w.x, (sx * c.u.y + sy * c.v.y) + c.w.y,
                                        (sx * c.u.z + sy * c.v.z) + c.w.z};
                    const float q = norm2(p);
                    bool lo = true, hi = true;
                    for (float a : p) {
                        lo = lo && std::fabs(a) >= 0x1p-100f;
                        hi = hi && std::fabs(a) <= 0x1p50f;
                        zero_num += a == 0.0f;
                    }
                    ++q_lo[q >= 0x1p-80f], ++q_hi[q < 0x1p40f], ++n_lo[lo], ++n_hi[hi];
                    ++((q >= 0x1p-80f && q < 0x1p40f && lo && hi) ? fast : general);
                }
                if (ci == 0 && step == 1u && h > 1u)  // the reference's camera: the oracle's primary ray
                    for (uint32_t i = 0; i < n; ++i) {
                        float r[3];
                        ref_primary_dir(i % w, i / w, w, h, r);
                        const F3 d = spt::camera_ray_dir(c, i % w, i / w, 0.0f, 0.0f, inv_w, inv_h, aspect);
                        const float dd[3] = {d.x, d.y, d.z};
                        if (r[0] == 0.0f || r[1] == 0.0f) continue;  // (a zero's sign may differ: DESIGN.md 3.8)
                        ++oracle_n;
                        oracle_bad += !same3(r, dd);
                    }
            }
            sec.n += n;
            if (g_host) continue;
            Dev<F3> out(n);
            k_camera<<<grid(n), 256>>>(c, w, step, n, inv_w, inv_h, aspect, seed, out.p);
            ran("k_camera");
            const std::vector<F3> got = out.get();
            for (uint32_t i = 0; i < n; ++i)
                if (!same3(&got[i].x, &want[i].x)) {
                    float jx, jy;
                    jitter_of(i, seed, jx, jy);
                    const float in[2] = {jx, jy};
                    sec.mismatch("camera " + cams[ci].name + " " + std::to_string(w) + "x" + std::to_string(h) + " pixel " +
                                 std::to_string(i % w) + "," + std::to_string((i / w) * step) + " jitter " + hex(in, 2) +
                                 " got " + hex(&got[i].x, 3) + " want " + hex(&want[i].x, 3));
                }
        }
    }
    if (oracle_bad) sec.mismatch("host build vs ref_primary_dir: " + std::to_string(oracle_bad) + " pixels");
    sec.need("fast", fast);
    sec.need("general", general);
    sec.need("q<2^-80", q_lo[0]);
    sec.need("q>=2^-80", q_lo[1]);
    sec.need("q>=2^40", q_hi[0]);
    sec.need("q<2^40", q_hi[1]);
    sec.need("num<2^-100", n_lo[0]);
    sec.need("num>=2^-100", n_lo[1]);
    sec.need("num>2^50", n_hi[0]);
    sec.need("num<=2^50", n_hi[1]);
    sec.need("zero_num", zero_num);
    sec.need("root_tie_cameras", root_ties);
    sec.need("vs_ref_primary_dir", oracle_n);
    return sec.report();
}

// ======================================================================================================
// 2. intersectors
// ======================================================================================================
struct Ray {
    float o[3], d[3];
};
struct PrimArg {
    float4 a, b, c, d;
    uint32_t type, fast_scene, rect, axis;  // axis: 1 + AX of an axis-aligned quad, else 0
};

// closest_flat's per-lane gate (spt_kernels.hip), restated: the loop sits in that file's anonymous
// namespace, and moving the predicate into a function of spt_device.h changed the kernels' machine code
__device__ bool flat_fast_ray_ok(F3 d, float a) {
    const float dmin = fminf(fminf(fabsf(d.x), fabsf(d.y)), fabsf(d.z));
    return dmin >= 0x1p-20f && a >= 0.5f && a <= 2.0f;
}

template <int AX>
__device__ float quad_fast(const PrimArg& P, F3 o, F3 d) {
    const spt::RcpRef r = spt::rcp_ref(spt::comp(d, AX));
    return P.rect ? spt::isect_quad_axis_fast<AX, true>(P.a, P.c, P.d, o, d, r, spt::kTNear)
                  : spt::isect_quad_axis_fast<AX, false>(P.a, P.c, P.d, o, d, r, spt::kTNear);
}

// fl: bit 0 the fast form was evaluated, bit 1 it set `redo`
__global__ void k_isect(PrimArg P, const Ray* rays, uint32_t n, float* t_general, float* t_fast, uint32_t* fl) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const F3 o{rays[i].o[0], rays[i].o[1], rays[i].o[2]}, d{rays[i].d[0], rays[i].d[1], rays[i].d[2]};
    t_general[i] = P.type == 0u   ? spt::isect_sphere(P.a, o, d, spt::kTNear)
                   : P.type == 1u ? spt::isect_quad(P.a, P.b, P.c, P.d, o, d, spt::kTNear)
                                  : spt::isect_tri(P.a, P.b, P.c, o, d, spt::kTNear);
    const float a = (d.x * d.x + d.y * d.y) + d.z * d.z;  // closest_flat's a
    float tf = 0.0f;
    uint32_t f = 0u;
    if (P.fast_scene && flat_fast_ray_ok(d, a) && (P.type == 0u || P.axis != 0u)) {
        f = 1u;
        if (P.type == 0u) {
            bool redo = false;
            tf = spt::isect_sphere_fast(P.a, P.b.x, o, d, a, spt::rcp_ref(2.0f * a), spt::kTNear, redo);
            f |= redo ? 2u : 0u;
        } else if (P.axis == 1u) {
            tf = quad_fast<0>(P, o, d);
        } else if (P.axis == 2u) {
            tf = quad_fast<1>(P, o, d);
        } else {
            tf = quad_fast<2>(P, o, d);
        }
    }
    t_fast[i] = tf;
    fl[i] = f;
}

struct IsectCounts {
    uint64_t fast = 0, redo = 0, disc0 = 0, disc_neg = 0, t1 = 0, t2 = 0, behind = 0;
    uint64_t gate_dmin = 0, gate_alo = 0, gate_ahi = 0, a_half = 0, a_two = 0, dmin_edge = 0, d_zero = 0;
    uint64_t tmin_in = 0, tmin_out = 0, root_tie = 0;
    uint64_t rect_lanes[3] = {0, 0, 0}, para_lanes[3] = {0, 0, 0}, general_quad = 0;
    uint64_t al_zero = 0, al_negzero = 0, al_one = 0, al_past_one = 0, al_below_zero = 0;
    uint64_t dax_zero_in = 0, dax_zero_off = 0, quad_hits = 0, quad_tmin_in = 0, quad_tmin_out = 0;
    uint64_t tri_hits = 0, tri_u0 = 0, tri_v0 = 0, tri_uv1 = 0, det0 = 0, det_lo_in = 0, det_lo_out = 0, det_hi_in = 0,
             det_hi_out = 0, tri_tmin_in = 0, tri_tmin_out = 0;
};

struct OneScene {
    std::string name;
    spt_prim prim{};
    std::vector<spt::DevPrim> dp, sorted;
    uint32_t rect_bits = 0;
    bool fast = false;
    ref_scene* rs = nullptr;
    std::vector<Ray> rays;
};

void make_scene(OneScene& s) {
    const spt_material mat{{0.7f, 0.7f, 0.7f}, {0, 0, 0}};
    const spt_env env{};
    const char* msg = nullptr;
    if (!spt::prepare_prims(&s.prim, 1, 1, s.dp, &msg)) {
        std::printf("prepare_prims refused %s: %s\n", s.name.c_str(), msg);
        std::exit(1);
    }
    uint32_t ends[spt::kFlatKinds - 1];
    spt::sort_flat_by_kind(s.dp, s.sorted, ends);
    s.rect_bits = spt::flat_rect_bits(s.sorted, ends);
    s.fast = spt::fast_division_ok(&s.prim, 1, s.dp);
    s.rs = ref_scene_create(&s.prim, 1, &mat, 1, &env);
}

inline void push_ray(std::vector<Ray>& r, const float o[3], const float d[3]) {
    r.push_back(Ray{{o[0], o[1], o[2]}, {d[0], d[1], d[2]}});
}
// o = p - t * d (fp32), then the ray
inline void push_through(std::vector<Ray>& r, const float p[3], const float d[3], float t) {
    const float o[3] = {p[0] - t * d[0], p[1] - t * d[1], p[2] - t * d[2]};
    push_ray(r, o, d);
}
// the 48 directions (+-1, +-0.5, +-0.25) in every order: exactly representable products and sums
inline void dyadic_dir(uint32_t k, float d[3]) {
    static const int perm[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
    const float m[3] = {1.0f, 0.5f, 0.25f};
    for (int c = 0; c < 3; ++c) d[c] = m[perm[k % 6u][c]] * (((k / 6u) >> c) & 1u ? -1.0f : 1.0f);
}

void sphere_rays(OneScene& s) {
    const float* C = s.prim.p0;
    const float r = C[3];
    std::vector<Ray>& R = s.rays;
    uint32_t h = bits(r) * 31u;
    // hashed rays aimed at the sphere's neighbourhood
    for (uint32_t i = 0; i < 20000u; ++i, h += 7u) {
        float o[3], t[3], d[3];
        for (int c = 0; c < 3; ++c) o[c] = C[c] + r * 3.0f * s11(h + c), t[c] = C[c] + r * 1.1f * s11(h + 3 + c);
        const float v[3] = {t[0] - o[0], t[1] - o[1], t[2] - o[2]};
        const float inv = 1.0f / std::sqrt(norm2(v));
        for (int c = 0; c < 3; ++c) d[c] = v[c] * inv;
        push_ray(R, o, d);
    }
    // the silhouette: the tangent direction from o (double, rounded once), then d.x moved by a few ulps
    for (uint32_t i = 0; i < 600u; ++i, h += 5u) {
        float e[3], f[3];
        unit3(h, e);
        unit3(h + 1u, f);
        const double dist = 1.5 + 3.0 * u01(h + 2u);  // |o - C| / r
        double L[3], P[3], pl = 0, dot = 0;
        for (int c = 0; c < 3; ++c) L[c] = -(double)e[c];  // unit, from o to C
        for (int c = 0; c < 3; ++c) dot += f[c] * L[c];
        for (int c = 0; c < 3; ++c) P[c] = f[c] - dot * L[c], pl += P[c] * P[c];
        pl = std::sqrt(pl);
        const double sn = 1.0 / dist, cs = std::sqrt(1.0 - sn * sn);
        float o[3], d0[3];
        for (int c = 0; c < 3; ++c) {
            o[c] = (float)((double)C[c] + (double)r * dist * e[c]);
            d0[c] = (float)(cs * L[c] + sn * P[c] / pl);
        }
        for (int k = -4; k <= 4; ++k) {
            const float d[3] = {ulps(d0[0], k), d0[1], d0[2]};
            push_ray(R, o, d);
        }
    }
    // origin on the surface, inside, at the centre
    for (uint32_t i = 0; i < 3000u; ++i, h += 3u) {
        float e[3], d[3], o[3];
        unit3(h, e);
        unit3(h + 1u, d);
        const float f = (i % 3u) == 0u ? 1.0f : ((i % 3u) == 1u ? 0.5f * u01(h + 2u) : 0.0f);
        for (int c = 0; c < 3; ++c) o[c] = C[c] + (r * f) * e[c];
        push_ray(R, o, d);
    }
    // a root next to tmin: from outside (the near root) and from inside (the far one)
    for (uint32_t i = 0; i < 400u; ++i, h += 3u) {
        float d[3];
        unit3(h, d);
        for (int k = -4; k <= 4; ++k) {
            const float t = ulps(spt::kTNear, k * 3);
            float o[3];
            for (int c = 0; c < 3; ++c) o[c] = C[c] - (r + t) * d[c];
            push_ray(R, o, d);
            for (int c = 0; c < 3; ++c) o[c] = C[c] + (r - t) * d[c];
            push_ray(R, o, d);
        }
    }
    // |d|^2 at 0.5 and 2 and their neighbours; a component at 2^-20, its neighbours and +-0
    const float small[7] = {0x1p-20f, 0x1.fffffep-21f, 0x1.000002p-20f, 0.0f, -0.0f, -0x1p-20f, 0x1.fffffep-21f * -1.0f};
    for (uint32_t k = 0; k < 8u * 3u * 7u; ++k) {
        const uint32_t sg = k & 7u, ax = (k >> 3) % 3u, e = k / 24u;
        for (int form = 0; form < 8; ++form) {
            float b[3];
            if (form < 3) b[0] = 0.5f, b[1] = ulps(0.5f, form - 1), b[2] = small[e];       // a = 0.5 -+
            else if (form < 6) b[0] = 1.0f, b[1] = ulps(1.0f, form - 4), b[2] = small[e];  // a = 2 -+
            else b[0] = form == 6 ? 0.6f : 0.28f, b[1] = form == 6 ? 0.8f : 0.96f, b[2] = small[e];
            float d[3];
            for (int c = 0; c < 3; ++c) d[(c + ax) % 3u] = b[c] * ((sg >> c) & 1u ? -1.0f : 1.0f);
            float p[3];
            for (int c = 0; c < 3; ++c) p[c] = C[c] + 0.25f * r * (float)((int)(k % 3u) - 1);
            push_through(R, p, d, 3.0f * r);
        }
    }
    // sqrt_unit's residual can only vanish for x next to an even power of two (x = s * pred(s) needs s or
    // pred(s) to be a power of two): origin at the centre, disc = 4 a r^2 with a next to 1. (On gfx950 the
    // hardware's estimate leaves no zero residual even there: `rm <= 0` and `rm < 0` give the same root for
    // every x of sqrt_unit's range, as tests/cpp/test_device_math.hip's exhaustive comparison shows for both.)
    const float near_one[3] = {0x1.fffffep-1f, 1.0f, 0x1.000002p0f};
    for (uint32_t k = 0; k < 60u; ++k) {
        float d[3];
        if (!find_norm2(near_one[k % 3u], 1000u + k, d)) continue;
        for (uint32_t sg = 0; sg < 2u; ++sg) {
            if (sg) d[0] = -d[0], d[2] = -d[2];
            push_ray(R, C, d);
        }
    }
    // a discriminant in (0, 2^-96) and around it (the `redo` protocol): a sphere at the origin whose radius is 5
    // units, o = (3, 4, lz) units on its surface with |lz| so small that the computed c is exactly 0, and
    // d = (+-1, -+0.75, dz): the first two products of L . d cancel exactly, b = 2 lz dz, disc = b * b
    if (C[0] == 0.0f && C[1] == 0.0f && C[2] == 0.0f) {
        const float lx = 3.0f * (r / 5.0f), ly = 4.0f * (r / 5.0f);
        if (lx * lx + ly * ly == r * r && lx == ly * 0.75f)
            for (int lk = 0; lk < 6; ++lk)
                for (int dk = 6; dk <= 20; ++dk)
                    for (uint32_t sg = 0; sg < 4u; ++sg) {
                        const float lz = lk == 5 ? 0.0f : std::ldexp(r, -12 - lk) * (sg & 1u ? -1.0f : 1.0f);
                        const float o[3] = {lx, ly, lz};
                        const float sx = sg & 2u ? -1.0f : 1.0f;
                        const float d[3] = {sx, -0.75f * sx, std::ldexp(1.0f, -dk)};
                        push_ray(R, o, d);
                    }
    }
}

void quad_rays(OneScene& s) {
    const float *Q = s.prim.p0, *u = s.prim.p1, *v = s.prim.p2;
    std::vector<Ray>& R = s.rays;
    const uint32_t axis = bits(s.dp[0].c[3]) >> spt::kMetaTypeBits;  // 1 + AX, 0: general
    const int AX = axis ? (int)axis - 1 : 2, U = AX == 0 ? 1 : 0, V = AX == 2 ? 1 : 2;
    // through the corners, the edge midpoints and the centre, and points one ulp to either side
    for (int ia = 0; ia < 3; ++ia)
        for (int ib = 0; ib < 3; ++ib)
            for (int su = -1; su <= 1; ++su)
                for (int sv = -1; sv <= 1; ++sv)
                    for (uint32_t k = 0; k < 48u; ++k)
                        for (float t : {2.0f, 4.0f}) {
                            float p[3], d[3];
                            for (int c = 0; c < 3; ++c) p[c] = (Q[c] + 0.5f * ia * u[c]) + 0.5f * ib * v[c];
                            p[U] = ulps(p[U], su);
                            p[V] = ulps(p[V], sv);
                            dyadic_dir(k, d);
                            push_through(R, p, d, t);
                        }
    float ctr[3];
    for (int c = 0; c < 3; ++c) ctr[c] = (Q[c] + 0.5f * u[c]) + 0.5f * v[c];
    if (axis) {
        // d[AX] = +-0 with the origin in the plane (0 / 0) and off it (+-inf)
        for (uint32_t k = 0; k < 12u; ++k) {
            float o[3] = {ctr[0] - 0.3f, ctr[1] - 0.3f, ctr[2] - 0.3f}, d[3];
            d[AX] = k & 1u ? -0.0f : 0.0f, d[U] = 0.6f, d[V] = 0.8f;
            o[AX] = Q[AX] + (float)((int)(k >> 1) % 3 - 1) * ((k >> 1) >= 3u ? 0x1p-20f : 1.0f);
            push_ray(R, o, d);
        }
        // t at tmin: d[AX] = +-1, o[AX] = Q[AX] -+ t for t around 0.001
        for (int k = -4; k <= 4; ++k)
            for (uint32_t sg = 0; sg < 2u; ++sg) {
                const float t = ulps(spt::kTNear, k);
                float o[3], d[3];
                d[AX] = sg ? -1.0f : 1.0f, d[U] = 0.25f, d[V] = -0.125f;
                for (int c = 0; c < 3; ++c) o[c] = ctr[c] - t * d[c];
                push_ray(R, o, d);
            }
    } else {
        // parallel to the plane (n . d = 0), in it and off it; t around tmin along the normal
        float n[3] = {u[1] * v[2] - v[1] * u[2], u[2] * v[0] - v[2] * u[0], u[0] * v[1] - v[0] * u[1]};
        for (uint32_t k = 0; k < 8u; ++k) {
            float o[3], d[3];
            for (int c = 0; c < 3; ++c) {
                d[c] = (k & 1u ? 0.25f * u[c] : 0.125f * v[c]) * (k & 2u ? -1.0f : 1.0f);
                o[c] = ctr[c] + (k & 4u ? 0.0f : 0.125f * n[c]);
            }
            push_ray(R, o, d);
        }
        for (int k = -4; k <= 4; ++k) {
            const float t = ulps(spt::kTNear, k * 2);
            const float d[3] = {n[0] * 0.0625f, n[1] * 0.0625f, n[2] * 0.0625f};
            push_through(R, ctr, d, t);
        }
    }
}

void tri_rays(OneScene& s, bool det_family) {
    const float *v0 = s.prim.p0, *v1 = s.prim.p1, *v2 = s.prim.p2;
    std::vector<Ray>& R = s.rays;
    float e1[3], e2[3], n[3];
    for (int c = 0; c < 3; ++c) e1[c] = v1[c] - v0[c], e2[c] = v2[c] - v0[c];
    n[0] = e1[1] * e2[2] - e2[1] * e1[2], n[1] = e1[2] * e2[0] - e2[2] * e1[0], n[2] = e1[0] * e2[1] - e2[0] * e1[1];
    // through the vertices, the edge midpoints and an inner point, and points one ulp to either side
    const float bary[7][2] = {{0, 0}, {1, 0}, {0, 1}, {0.5f, 0}, {0, 0.5f}, {0.5f, 0.5f}, {0.25f, 0.25f}};
    for (const auto& b : bary)
        for (int sx = -1; sx <= 1; ++sx)
            for (int sy = -1; sy <= 1; ++sy)
                for (uint32_t k = 0; k < 48u; ++k)
                    for (float t : {2.0f, 4.0f}) {
                        float p[3], d[3];
                        for (int c = 0; c < 3; ++c) p[c] = (v0[c] + b[0] * e1[c]) + b[1] * e2[c];
                        p[0] = ulps(p[0], sx);
                        p[1] = ulps(p[1], sy);
                        dyadic_dir(k, d);
                        push_through(R, p, d, t);
                    }
    // along the edges, in the triangle's plane and beside it: det = 0
    for (uint32_t k = 0; k < 24u; ++k) {
        float o[3], d[3];
        const uint32_t edge = k % 3u;
        for (int c = 0; c < 3; ++c) {
            const float ed = edge == 0u ? e1[c] : (edge == 1u ? e2[c] : e2[c] - e1[c]);
            const float from = edge == 2u ? v1[c] : v0[c];
            d[c] = ed * (k & 4u ? -0.25f : 0.25f);
            o[c] = (from - d[c]) + (k & 8u ? 0.125f * n[c] : 0.0f) + (k & 16u ? 0.0625f * e1[c] : 0.0f);
        }
        push_ray(R, o, d);
    }
    float inner[3];
    for (int c = 0; c < 3; ++c) inner[c] = (v0[c] + 0.25f * e1[c]) + 0.25f * e2[c];
    if (det_family) {
        // a triangle in the plane z = 0 with e1 x e2 = (0, 0, 4): det = -4 d.z, at the edges of recip_ref's fast
        // range [2^-40, 2^20), outside it, and denormal
        const float dz[9] = {0x1p-42f, 0x1.fffffep-43f, 0x1.000002p-42f, 0x1p18f, 0x1.fffffep17f, 0x1.000002p18f,
                             0x1p-60f, 0x1p40f, 0x1p-140f};
        for (float z : dz)
            for (uint32_t sg = 0; sg < 4u; ++sg) {
                const float d[3] = {sg & 2u ? -0.25f : 0.25f, 0.125f, sg & 1u ? -z : z};
                push_through(R, inner, d, 1.0f);
            }
    }
    // t around tmin, along the normal
    for (int k = -4; k <= 4; ++k)
        for (uint32_t sg = 0; sg < 2u; ++sg) {
            const float t = ulps(spt::kTNear, k);
            const float f = sg ? -0.25f : 0.25f;
            const float d[3] = {n[0] * f, n[1] * f, n[2] * f};
            push_through(R, inner, d, t);
        }
}

// the branch each ray reaches, from the host's evaluation of the same expressions (counters only)
void count_sphere(const OneScene& s, const Ray& ray, bool gate, float disc, IsectCounts& k) {
    const float* d = ray.d;
    const float a = norm2(d);
    const float dmin = std::fmin(std::fmin(std::fabs(d[0]), std::fabs(d[1])), std::fabs(d[2]));
    k.gate_dmin += dmin < 0x1p-20f;
    k.gate_alo += a < 0.5f;
    k.gate_ahi += a > 2.0f;
    k.a_half += a == 0.5f && gate;
    k.a_two += a == 2.0f && gate;
    k.dmin_edge += dmin == 0x1p-20f && gate;
    k.d_zero += dmin == 0.0f;
    k.disc0 += disc == 0.0f;
    k.disc_neg += disc < 0.0f;
    if (disc >= 0.0f) {
        const float lx = ray.o[0] - s.prim.p0[0], ly = ray.o[1] - s.prim.p0[1], lz = ray.o[2] - s.prim.p0[2];
        const float b = 2.0f * ((lx * d[0] + ly * d[1]) + lz * d[2]);
        const float sq = std::sqrt(disc), t1 = (-b - sq) / (2.0f * a), t2 = (-b + sq) / (2.0f * a);
        const float lo = ulps(spt::kTNear, -64), hi = ulps(spt::kTNear, 64);
        for (float t : {t1, t2}) {
            k.tmin_in += t >= spt::kTNear && t <= hi;
            k.tmin_out += t < spt::kTNear && t >= lo;
        }
        if (t1 >= spt::kTNear) ++k.t1;
        else if (t2 >= spt::kTNear) ++k.t2;
        else ++k.behind;
        // disc next to an even power of two: sqrtf's last correction has a zero residual
        const uint32_t m = bits(disc) & 0x7fffffu, e = bits(disc) >> 23;
        k.root_tie += gate && ((m == 0x7fffffu && (e & 1u) == 0u) || (m == 1u && (e & 1u) == 1u));
    }
}

void count_quad(const OneScene& s, const Ray& ray, bool gate, IsectCounts& k) {
    const spt::DevPrim& p = s.dp[0];
    const uint32_t axis = bits(p.c[3]) >> spt::kMetaTypeBits;
    if (!axis) {
        ++k.general_quad;
        return;
    }
    const int AX = (int)axis - 1, U = AX == 0 ? 1 : 0, V = AX == 2 ? 1 : 2;
    const float* o = ray.o;
    const float* d = ray.d;
    if (d[AX] == 0.0f) {
        ++(o[AX] == p.a[AX] ? k.dax_zero_in : k.dax_zero_off);
        return;
    }
    if (gate) ++((s.rect_bits >> AX) & 1u ? k.rect_lanes[AX] : k.para_lanes[AX]);
    const float t = (p.a[AX] - o[AX]) / d[AX];
    k.quad_tmin_in += t >= spt::kTNear && t <= ulps(spt::kTNear, 8);
    k.quad_tmin_out += t < spt::kTNear && t >= ulps(spt::kTNear, -8);
    if (!(t >= spt::kTNear) || t == INFINITY) return;
    const float hu = (o[U] + t * d[U]) - p.a[U], hv = (o[V] + t * d[V]) - p.a[V];
    // the axis form's sums and the rectangle form's single products
    const float forms[4] = {hu * p.c[U] + hv * p.c[V], hu * p.d[U] + hv * p.d[V], hu * p.c[U], hv * p.d[V]};
    const bool rect = (s.rect_bits >> AX) & 1u;
    for (int f = 0; f < (rect ? 4 : 2); ++f) {
        const float x = forms[f];
        k.al_zero += bits(x) == 0u;
        k.al_negzero += bits(x) == 0x80000000u;
        k.al_one += x == 1.0f;
        k.al_past_one += x > 1.0f && x <= 0x1.00001p0f;
        k.al_below_zero += x < 0.0f && x >= -0x1p-20f;
    }
}

void count_tri(const OneScene& s, const Ray& ray, float want_t, IsectCounts& k) {
    const spt::DevPrim& p = s.dp[0];
    const float *o = ray.o, *d = ray.d, *e1 = p.b, *e2 = p.c;
    const float px = d[1] * e2[2] - e2[1] * d[2], py = d[2] * e2[0] - e2[2] * d[0], pz = d[0] * e2[1] - e2[0] * d[1];
    const float det = (e1[0] * px + e1[1] * py) + e1[2] * pz, ad = std::fabs(det);
    k.det0 += det == 0.0f;
    k.det_lo_in += ad >= 0x1p-40f && ad < 0x1.1p-40f;
    k.det_lo_out += ad > 0.0f && ad < 0x1p-40f;
    k.det_hi_in += ad >= 0x1.ep19f && ad < 0x1p20f;
    k.det_hi_out += ad >= 0x1p20f;
    const float inv = 1.0f / det;
    const float tx = o[0] - p.a[0], ty = o[1] - p.a[1], tz = o[2] - p.a[2];
    const float u = ((tx * px + ty * py) + tz * pz) * inv;
    const float qx = ty * e1[2] - e1[1] * tz, qy = tz * e1[0] - e1[2] * tx, qz = tx * e1[1] - e1[0] * ty;
    const float v = ((d[0] * qx + d[1] * qy) + d[2] * qz) * inv;
    k.tri_u0 += u == 0.0f;
    k.tri_v0 += v == 0.0f && u >= 0.0f && u <= 1.0f;
    k.tri_uv1 += u >= 0.0f && v >= 0.0f && u + v == 1.0f;
    k.tri_hits += want_t < INFINITY;
    const float t = ((e2[0] * qx + e2[1] * qy) + e2[2] * qz) * inv;
    if (u >= 0.0f && v >= 0.0f && u + v <= 1.0f) {
        k.tri_tmin_in += t >= spt::kTNear && t <= ulps(spt::kTNear, 8);
        k.tri_tmin_out += t < spt::kTNear && t >= ulps(spt::kTNear, -8);
    }
}

bool check_intersectors() {
    Section sec("intersect");
    std::vector<OneScene> scenes;
    auto sphere = [&](const char* nm, float x, float y, float z, float r) {
        OneScene s;
        s.name = nm;
        s.prim.type = SPT_PRIM_SPHERE;
        s.prim.p0[0] = x, s.prim.p0[1] = y, s.prim.p0[2] = z, s.prim.p0[3] = r;
        make_scene(s);
        sphere_rays(s);
        scenes.push_back(std::move(s));
    };
    sphere("sphere r=2^-20", 0, 0, 0, 0x1p-20f);
    sphere("sphere r=5*2^-22", 0, 0, 0, 0x1.4p-20f);  // (beside the four radii: the one that reaches `redo`)
    sphere("sphere r=1", 1, -2, 5, 1.0f);
    sphere("sphere r=100", -30, 60, 200, 100.0f);
    sphere("sphere r=2^27", 0x1p20f, -0x1p21f, 0x1p26f, 0x1p27f);
    auto flat3 = [&](const char* nm, uint32_t type, const float a[3], const float b[3], const float c[3], bool detf) {
        OneScene s;
        s.name = nm;
        s.prim.type = type;
        for (int k = 0; k < 3; ++k) s.prim.p0[k] = a[k], s.prim.p1[k] = b[k], s.prim.p2[k] = c[k];
        make_scene(s);
        if (type == SPT_PRIM_QUAD) quad_rays(s);
        else tri_rays(s, detf);
        scenes.push_back(std::move(s));
    };
    static const char* rect_names[3] = {"rectangle x", "rectangle y", "rectangle z"};
    static const char* para_names[3] = {"parallelogram x", "parallelogram y", "parallelogram z"};
    for (int AX = 0; AX < 3; ++AX) {
        const int U = AX == 0 ? 1 : 0, V = AX == 2 ? 1 : 2;
        float Q[3], u[3] = {0, 0, 0}, v[3] = {0, 0, 0};
        // a rectangle in the plane x[AX] = 0 whose first edge runs in the negative direction (a zero hit
        // coordinate times the negative edge-basis term is -0)
        Q[AX] = 0.0f, Q[U] = 1.0f, Q[V] = -2.0f, u[U] = -2.0f, v[V] = 4.0f;
        flat3(rect_names[AX], SPT_PRIM_QUAD, Q, u, v, false);
        // an in-plane parallelogram, |u x v| = 8 (exact edge basis)
        Q[AX] = 3.0f, Q[U] = -1.0f, Q[V] = 0.5f, u[U] = 2.0f, u[V] = 2.0f, v[U] = -2.0f, v[V] = 2.0f;
        flat3(para_names[AX], SPT_PRIM_QUAD, Q, u, v, false);
    }
    {
        const float Q[3] = {1, -1, 2}, u[3] = {2, 0, 2}, v[3] = {0, 4, 0};
        flat3("general quad", SPT_PRIM_QUAD, Q, u, v, false);
        const float a[3] = {-1, -1, 0}, b[3] = {1, -1, 0}, c[3] = {-1, 1, 0};
        flat3("triangle z=0", SPT_PRIM_TRIANGLE, a, b, c, true);
        const float a2[3] = {1, -1, 2}, b2[3] = {3, -1, 4}, c2[3] = {1, 3, 2};
        flat3("general triangle", SPT_PRIM_TRIANGLE, a2, b2, c2, false);
    }

    IsectCounts k;
    uint64_t fast_scenes = 0;
    for (OneScene& s : scenes) {
        const uint32_t n = (uint32_t)s.rays.size();
        const spt::DevPrim& p = s.sorted[0];  // the kind-major copy, which the fast forms read
        const uint32_t type = s.prim.type, axis = type == SPT_PRIM_QUAD ? bits(p.c[3]) >> spt::kMetaTypeBits : 0u;
        fast_scenes += s.fast;
        std::vector<float> want(n), disc(n, -1.0f);
        std::vector<uint32_t> want_fl(n, 0u);
        {
            Clock clk;
            for (uint32_t i = 0; i < n; ++i) {
                const Ray& r = s.rays[i];
                float t = INFINITY;
                uint32_t prim = 0;
                if (!ref_intersect(s.rs, r.o, r.d, 0.001f, &t, &prim, nullptr)) t = INFINITY;
                want[i] = t;
            }
        }
        for (uint32_t i = 0; i < n; ++i) {
            const Ray& r = s.rays[i];
            // closest_flat's per-lane gate once more, on the host
            const float a = norm2(r.d);
            const float dmin = std::fmin(std::fmin(std::fabs(r.d[0]), std::fabs(r.d[1])), std::fabs(r.d[2]));
            const bool gate = s.fast && dmin >= 0x1p-20f && a >= 0.5f && a <= 2.0f && (type == SPT_PRIM_SPHERE || axis);
            want_fl[i] = gate ? 1u : 0u;
            k.fast += gate;
            if (type == SPT_PRIM_SPHERE) {
                // isect_sphere_fast's discriminant, the same expression (rr: the host's product)
                const float lx = r.o[0] - p.a[0], ly = r.o[1] - p.a[1], lz = r.o[2] - p.a[2];
                const float b = 2.0f * ((lx * r.d[0] + ly * r.d[1]) + lz * r.d[2]);
                const float c = ((lx * lx + ly * ly) + lz * lz) - p.b[0];
                disc[i] = b * b - 4.0f * a * c;
                if (gate && disc[i] > 0.0f && disc[i] < 0x1p-96f) want_fl[i] |= 2u, ++k.redo;
                count_sphere(s, r, gate, disc[i], k);
            } else if (type == SPT_PRIM_QUAD) {
                count_quad(s, r, gate, k);
                k.quad_hits += want[i] < INFINITY;
            } else {
                count_tri(s, r, want[i], k);
            }
        }
        sec.n += n;
        if (g_host) continue;
        PrimArg P;
        P.a = make_float4(p.a[0], p.a[1], p.a[2], p.a[3]);
        P.b = make_float4(p.b[0], p.b[1], p.b[2], p.b[3]);
        P.c = make_float4(p.c[0], p.c[1], p.c[2], p.c[3]);
        P.d = make_float4(p.d[0], p.d[1], p.d[2], p.d[3]);
        P.type = type, P.fast_scene = s.fast, P.axis = axis, P.rect = axis ? (s.rect_bits >> (axis - 1u)) & 1u : 0u;
        Dev<Ray> rays(s.rays);
        Dev<float> tg(n), tf(n);
        Dev<uint32_t> fl(n);
        k_isect<<<grid(n), 256>>>(P, rays.p, n, tg.p, tf.p, fl.p);
        ran("k_isect");
        const std::vector<float> g = tg.get(), f = tf.get();
        const std::vector<uint32_t> gf = fl.get();
        for (uint32_t i = 0; i < n; ++i) {
            const char* what = nullptr;
            if (!same(g[i], want[i])) what = "general form";
            else if (gf[i] != want_fl[i]) what = (gf[i] ^ want_fl[i]) & 2u ? "redo flag" : "gate";
            // a lane that set redo is answered by the general form, as in closest_flat
            else if ((gf[i] & 3u) == 1u && !same(f[i], want[i])) what = "fast form";
            if (what)
                sec.mismatch(s.name + " ray " + std::to_string(i) + " (" + what + ") o " + hex(s.rays[i].o, 3) + " d " +
                             hex(s.rays[i].d, 3) + " general " + hex(&g[i], 1) + " fast " + hex(&f[i], 1) + " flags " +
                             std::to_string(gf[i]) + "/" + std::to_string(want_fl[i]) + " want " + hex(&want[i], 1));
        }
    }
    for (OneScene& s : scenes) ref_scene_destroy(s.rs);
    sec.need("fast_scenes", fast_scenes);
    sec.need("fast", k.fast);
    sec.need("redo", k.redo);
    sec.need("disc=0", k.disc0);
    sec.need("disc<0", k.disc_neg);
    sec.need("t1", k.t1);
    sec.need("t2", k.t2);
    sec.need("behind", k.behind);
    sec.need("root~tmin+", k.tmin_in);
    sec.need("root~tmin-", k.tmin_out);
    sec.need("root_tie", k.root_tie);
    sec.need("dmin<2^-20", k.gate_dmin);
    sec.need("dmin=2^-20", k.dmin_edge);
    sec.need("d=0", k.d_zero);
    sec.need("a<.5", k.gate_alo);
    sec.need("a=.5", k.a_half);
    sec.need("a=2", k.a_two);
    sec.need("a>2", k.gate_ahi);
    for (int ax = 0; ax < 3; ++ax) {
        sec.need(ax == 0 ? "rect_x" : (ax == 1 ? "rect_y" : "rect_z"), k.rect_lanes[ax]);
        sec.need(ax == 0 ? "para_x" : (ax == 1 ? "para_y" : "para_z"), k.para_lanes[ax]);
    }
    sec.need("general_quad", k.general_quad);
    sec.need("quad_hits", k.quad_hits);
    sec.need("alpha=+0", k.al_zero);
    sec.need("alpha=-0", k.al_negzero);
    sec.need("alpha=1", k.al_one);
    sec.need("alpha>1", k.al_past_one);
    sec.need("alpha<0", k.al_below_zero);
    sec.need("dAX=0_in_plane", k.dax_zero_in);
    sec.need("dAX=0_off_plane", k.dax_zero_off);
    sec.need("quad_t~tmin+", k.quad_tmin_in);
    sec.need("quad_t~tmin-", k.quad_tmin_out);
    sec.need("tri_hits", k.tri_hits);
    sec.need("tri_u=0", k.tri_u0);
    sec.need("tri_v=0", k.tri_v0);
    sec.need("tri_u+v=1", k.tri_uv1);
    sec.need("det=0", k.det0);
    sec.need("det>=2^-40", k.det_lo_in);
    sec.need("det<2^-40", k.det_lo_out);
    sec.need("det<2^20", k.det_hi_in);
    sec.need("det>=2^20", k.det_hi_out);
    sec.need("tri_t~tmin+", k.tri_tmin_in);
    sec.need("tri_t~tmin-", k.tri_tmin_out);
    return sec.report();
}

// ======================================================================================================
// 3. sincos and bounce
// ======================================================================================================
__global__ void k_sincos(const float* phi, uint32_t n, double* out) {  // out: s<false>, c<false>, s<true>, c<true>
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double s, c;
    spt::sincos_2pi<false>((double)phi[i], s, c);
    out[4 * (size_t)i + 0] = s;
    out[4 * (size_t)i + 1] = c;
    spt::sincos_2pi<true>((double)phi[i], s, c);
    out[4 * (size_t)i + 2] = s;
    out[4 * (size_t)i + 3] = c;
}

struct BounceIn {
    float n[3];
    uint32_t state, flags;
};
struct BounceOut {
    float d0[3], d1[3];  // <false>, <true>
    uint32_t s0, s1;
};
__global__ void k_bounce(const BounceIn* in, uint32_t n, BounceOut* out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const F3 nn{in[i].n[0], in[i].n[1], in[i].n[2]};
    uint32_t s0 = in[i].state, s1 = in[i].state;
    const F3 a = spt::bounce_dir<false>(nn, s0, in[i].flags), b = spt::bounce_dir<true>(nn, s1, in[i].flags);
    out[i] = BounceOut{{a.x, a.y, a.z}, {b.x, b.y, b.z}, s0, s1};
}

// sincos_2pi with ONE of its Horner steps (the index of the coefficient it adds) as a separate multiply and
// add: says on the host which inputs can tell a step that lost its fusion. Over every float in [2^-7, 2 pi]
// steps 2, 3, 9, 10 and 11 change no result at all, step 4 changes 3 results, step 12 changes 6, steps 5, 6, 13
// and 14 more: kFusionSensitive lists all of the former and a dozen of each of the latter.
void sincos_one_step_unfused(double phi, int unfused, double& s, double& c) {
    static const double cf[16] = {SPT_SINCOS_COEFS, 0.0};
    const double k = __builtin_rint(phi * 6.36619772367581382433e-01);
    const double r = (phi - k * 1.57079632679489655800e+00) - k * 6.12323399573676603587e-17;
    const double w = r * r;
    auto step = [&](double p, int i) { return i == unfused ? p * w + cf[i] : __builtin_fma(p, w, cf[i]); };
    double ps = __builtin_fma(cf[0], w, cf[1]);
    for (int i = 2; i <= 6; ++i) ps = step(ps, i);
    const double sr = __builtin_fma(r * w, ps, r);
    double pc = __builtin_fma(cf[7], w, cf[8]);
    for (int i = 9; i <= 14; ++i) pc = step(pc, i);
    const double cr = __builtin_fma(w, pc, 1.0);
    const int q = ((int)k) & 3;
    const double a = (q & 1) ? cr : sr, b = (q & 1) ? sr : cr;
    s = (q & 2) ? -a : a;
    c = ((q + 1) & 2) ? -b : b;
}
struct FusionCase {
    int step;
    uint32_t phi_bits;
};
const FusionCase kFusionSensitive[] = {
    {4, 0x3f2e9476}, {4, 0x3f413d85}, {4, 0x3f617e40},
    {5, 0x3f03b7a4}, {5, 0x3f0ff701}, {5, 0x3f1ca3e9}, {5, 0x3f2387f1}, {5, 0x3f24bf72}, {5, 0x3f27c84c},
    {5, 0x3f28eafc}, {5, 0x3f28ebbd}, {5, 0x3f298b87}, {5, 0x3f2a10e2}, {5, 0x3f2a551a}, {5, 0x3f2d1506},
    {6, 0x3d6c4e76}, {6, 0x3dbd205e}, {6, 0x3dd36e65}, {6, 0x3dedc587}, {6, 0x3e0a5e53}, {6, 0x3e14703f},
    {6, 0x3e16d09f}, {6, 0x3e224cc2}, {6, 0x3e25715c}, {6, 0x3f4126ea}, {6, 0x3f72953f}, {6, 0x407a450e},
    {12, 0x3f345f65}, {12, 0x3f43cc84}, {12, 0x3f577010}, {12, 0x3f5b3168}, {12, 0x3f5dc16a}, {12, 0x3f6d242c},
    {13, 0x3e3a8d85}, {13, 0x3e67d600}, {13, 0x3e9ae573}, {13, 0x3ead400c}, {13, 0x3ebd712d}, {13, 0x3ec7acd0},
    {13, 0x3ec7fc36}, {13, 0x3ecb3f29}, {13, 0x3ed0f6e5}, {13, 0x3ed53887}, {13, 0x3ed70e84}, {13, 0x3ed76207},
    {14, 0x3d54af96}, {14, 0x3da331b8}, {14, 0x3dac350a}, {14, 0x3ee96f8b}, {14, 0x3f0a937e}, {14, 0x3f5624e9},
    {14, 0x3f8000cd}, {14, 0x400496e0}, {14, 0x402202c3}, {14, 0x407110ad}, {14, 0x408094bb}, {14, 0x40b457d1},
};

bool check_sincos() {
    Section sec("sincos");
    std::vector<float> phi;
    uint64_t boundary = 0, quadrant[4] = {0, 0, 0, 0};
    phi.push_back(2.0f * spt::kPiF * 0.0f);
    phi.push_back(2.0f * spt::kPiF * 1.0f);
    // u2 around every multiple of 1/8: phi around k pi/2 (an exact reduction) and around (k + 1/2) pi/2 (where
    // the quadrant switches), 4 ulps to either side
    for (int m = 0; m <= 8; ++m)
        for (int k = -4; k <= 4; ++k) {
            const float u2 = ulps(0.125f * (float)m, k);
            if (!(u2 >= 0.0f && u2 <= 1.0f)) continue;
            phi.push_back(2.0f * spt::kPiF * u2);
            ++boundary;
        }
    // the inputs at which the fusion of one Horner step decides the result (a step computed as a multiply and
    // an add is otherwise invisible: 2^22 draws meet none of step 4's three inputs)
    uint64_t sensitive[15] = {0}, restated_bad = 0;
    for (const FusionCase& f : kFusionSensitive) {
        double s0, c0, s1, c1;
        spt::sincos_2pi<false>((double)fbits(f.phi_bits), s0, c0);
        sincos_one_step_unfused((double)fbits(f.phi_bits), f.step, s1, c1);
        sensitive[f.step] += !same(s0, s1) || !same(c0, c1);
        sincos_one_step_unfused((double)fbits(f.phi_bits), -1, s1, c1);
        restated_bad += !same(s0, s1) || !same(c0, c1);
        phi.push_back(fbits(f.phi_bits));
    }
    if (restated_bad) sec.mismatch("sincos_one_step_unfused with every step fused is not sincos_2pi's host build");
    uint64_t all_sensitive = 0;
    for (uint64_t v : sensitive) all_sensitive += v;
    if (all_sensitive != sizeof(kFusionSensitive) / sizeof(kFusionSensitive[0]))
        sec.mismatch("a kFusionSensitive input does not depend on its step's fusion");
    for (uint32_t i = 0; i < (1u << 22); ++i) {
        uint32_t state = i * 1021u + 12345u;
        phi.push_back(2.0f * spt::kPiF * spt::random_float(state));
    }
    const uint32_t n = (uint32_t)phi.size();
    std::vector<double> want(2 * (size_t)n);
    {
        Clock clk;
        for (uint32_t i = 0; i < n; ++i) {
            spt::sincos_2pi<false>((double)phi[i], want[2 * (size_t)i], want[2 * (size_t)i + 1]);
            ++quadrant[(int)__builtin_rint((double)phi[i] * 6.36619772367581382433e-01) & 3];
        }
    }
    sec.n = n;
    if (!g_host) {
        Dev<float> dphi(phi);
        Dev<double> out(4 * (size_t)n);
        k_sincos<<<grid(n), 256>>>(dphi.p, n, out.p);
        ran("k_sincos");
        const std::vector<double> got = out.get();
        for (uint32_t i = 0; i < n; ++i)
            for (int v = 0; v < 2; ++v)
                if (!same(got[4 * (size_t)i + 2 * v], want[2 * (size_t)i]) ||
                    !same(got[4 * (size_t)i + 2 * v + 1], want[2 * (size_t)i + 1])) {
                    char b[200];
                    std::snprintf(b, sizeof b, "sincos_2pi<%s> phi %08x got %a %a want %a %a", v ? "true" : "false",
                                  bits(phi[i]), got[4 * (size_t)i + 2 * v], got[4 * (size_t)i + 2 * v + 1],
                                  want[2 * (size_t)i], want[2 * (size_t)i + 1]);
                    sec.mismatch(b);
                }
    }
    sec.need("boundary", boundary);
    for (int st : {4, 5, 6, 12, 13, 14}) sec.need(("fusion_step" + std::to_string(st)).c_str(), sensitive[st]);
    for (int q = 0; q < 4; ++q) sec.need(q == 0 ? "k=0|4" : (q == 1 ? "k=1" : (q == 2 ? "k=2" : "k=3")), quadrant[q]);
    return sec.report();
}

bool check_bounce() {
    Section sec("bounce");
    const uint32_t n = 1u << 20;
    std::vector<BounceIn> in(n);
    uint64_t pole[2][2] = {{0, 0}, {0, 0}}, zero_z = 0, axis_n = 0, host_bad = 0;
    for (uint32_t i = 0; i < n; ++i) {
        BounceIn& b = in[i];
        b.state = hash32(i * 3u + 1u);
        b.flags = (i >> 3) & 1u ? SPT_FLAG_ABS_FLOAT : 0u;
        const uint32_t fam = i & 7u, v = i >> 4;
        if (fam < 4u) {
            unit3(i, b.n);
        } else if (fam == 4u) {  // the axis normals
            b.n[0] = b.n[1] = b.n[2] = 0.0f;
            b.n[v % 3u] = (v / 3u) & 1u ? -1.0f : 1.0f;
            ++axis_n;
        } else if (fam == 5u) {  // n.z = +-0
            const double a = 6.283185307179586 * u01(i);
            b.n[0] = (float)std::cos(a), b.n[1] = (float)std::sin(a), b.n[2] = v & 1u ? -0.0f : 0.0f;
            ++zero_z;
        } else {  // |n.z| on either side of bounce_tangent's switch: 0.999f (fabsf) and 1.0f ((int)n.z)
            const float z = ulps(fam == 6u ? 0.999f : 1.0f, (int)(v % 9u) - (fam == 6u ? 4 : 8));
            const float s = std::sqrt(std::fmax(1.0f - z * z, 0.0f));
            const double a = 6.283185307179586 * u01(i);
            b.n[0] = s * (float)std::cos(a), b.n[1] = s * (float)std::sin(a), b.n[2] = (v / 9u) & 1u ? -z : z;
        }
        const bool not_pole = b.flags ? std::fabs(b.n[2]) < 0.999f : (int)b.n[2] == 0;
        ++pole[b.flags ? 1 : 0][not_pole];
    }
    std::vector<BounceOut> want(n);
    {
        Clock clk;
        for (uint32_t i = 0; i < n; ++i) {
            uint32_t s = in[i].state;
            ref_bounce_dir(in[i].n, &s, in[i].flags, want[i].d0);
            want[i].s0 = s;
            // the host build
            uint32_t hs = in[i].state;
            const F3 h = spt::bounce_dir<false>(F3{in[i].n[0], in[i].n[1], in[i].n[2]}, hs, in[i].flags);
            if (!same3(&h.x, want[i].d0) || hs != s) {
                if (!host_bad++)
                    sec.mismatch("host build, n " + hex(in[i].n, 3) + " state " + hexu(in[i].state) + " flags " +
                                 std::to_string(in[i].flags) + " got " + hex(&h.x, 3) + " want " + hex(want[i].d0, 3));
            }
        }
    }
    sec.n = n;
    if (!g_host) {
        Dev<BounceIn> din(in);
        Dev<BounceOut> out(n);
        k_bounce<<<grid(n), 256>>>(din.p, n, out.p);
        ran("k_bounce");
        const std::vector<BounceOut> got = out.get();
        for (uint32_t i = 0; i < n; ++i)
            if (!same3(got[i].d0, want[i].d0) || !same3(got[i].d1, want[i].d0) || got[i].s0 != want[i].s0 ||
                got[i].s1 != want[i].s0)
                sec.mismatch("n " + hex(in[i].n, 3) + " state " + hexu(in[i].state) + " flags " + std::to_string(in[i].flags) +
                             " <false> " + hex(got[i].d0, 3) + " <true> " + hex(got[i].d1, 3) + " want " +
                             hex(want[i].d0, 3));
    }
    sec.need("int_pole", pole[0][0]);
    sec.need("int_not_pole", pole[0][1]);
    sec.need("fabs_pole", pole[1][0]);
    sec.need("fabs_not_pole", pole[1][1]);
    sec.need("axis_normals", axis_n);
    sec.need("n.z=+-0", zero_z);
    return sec.report();
}

// ======================================================================================================
// 4. BSDF step
// ======================================================================================================
struct BsdfIn {
    float d[3], nf[3], param;
    uint32_t kind, entering, flags, state;
};
struct BsdfOut {
    float d0[3], d1[3];
    uint32_t f0, f1, s0, s1;  // f: transmitted | absorbed << 1
};
__global__ void k_bsdf(const BsdfIn* in, uint32_t n, BsdfOut* out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const BsdfIn x = in[i];
    const F3 d{x.d[0], x.d[1], x.d[2]}, nf{x.nf[0], x.nf[1], x.nf[2]};
    uint32_t s0 = x.state, s1 = x.state;
    const spt::Scatter a = spt::bsdf_scatter<false>(x.kind, x.param, d, nf, x.entering != 0u, x.flags, s0);
    const spt::Scatter b = spt::bsdf_scatter<true>(x.kind, x.param, d, nf, x.entering != 0u, x.flags, s1);
    out[i] = BsdfOut{{a.dir.x, a.dir.y, a.dir.z}, {b.dir.x, b.dir.y, b.dir.z},
                     (a.transmitted ? 1u : 0u) | (a.absorbed ? 2u : 0u), (b.transmitted ? 1u : 0u) | (b.absorbed ? 2u : 0u),
                     s0, s1};
}

bool check_bsdf() {
    Section sec("bsdf");
    const uint32_t n = 1u << 18;
    std::vector<BsdfIn> in(n);
    uint64_t tir = 0, k_one = 0, k_near = 0, transmit = 0, reflect = 0, absorbed = 0, cancel = 0, ior1 = 0, normal_inc = 0,
             enter[2] = {0, 0}, grazing = 0, fuzz[3] = {0, 0, 0};
    const float iors[6] = {1.0f, 1.33f, 1.5f, 2.4f, 0.75f, 0.0f};
    for (uint32_t i = 0; i < n; ++i) {
        BsdfIn& x = in[i];
        const uint32_t mode = i & 7u, v = i >> 3, h = hash32(i + 0xb5d1u);
        x.state = hash32(i * 5u + 3u);
        x.flags = h & 1u ? SPT_FLAG_ABS_FLOAT : 0u;
        x.entering = (h >> 1) & 1u;
        x.kind = v & 1u ? SPT_MAT_DIELECTRIC : SPT_MAT_METAL;
        const uint32_t pick = (h >> 4) % 6u;
        if (x.kind == SPT_MAT_METAL) x.param = pick == 0u ? 0.0f : (pick == 1u ? 1.0f : u01(h + 9u));
        else x.param = pick == 5u ? 0.3f + 2.7f * u01(h + 9u) : iors[pick];
        unit3(i, x.nf);
        float d[3];
        unit3(i + 0x40000000u, d);
        if (mode == 0u) {  // grazing: almost in the tangent plane, now and then just past it
            float t[3] = {x.nf[1] * d[2] - d[1] * x.nf[2], x.nf[2] * d[0] - d[2] * x.nf[0], x.nf[0] * d[1] - d[0] * x.nf[1]};
            const double tl = std::sqrt((double)norm2(t));
            const double eps = std::pow(10.0, -7.0 + 6.0 * u01(h + 5u)) * ((v % 10u) ? -1.0 : 1.0);
            double w[3], wl = 0;
            for (int c = 0; c < 3; ++c) w[c] = t[c] / tl + eps * x.nf[c], wl += w[c] * w[c];
            for (int c = 0; c < 3; ++c) x.d[c] = (float)(w[c] / std::sqrt(wl));
            ++grazing;
        } else if (mode == 4u) {  // DIELECTRIC with k = eta^2 (1 - ci^2) within a few ulps of 1: axis normal, so
            // that -dot(d, nf) is the ci chosen
            x.kind = SPT_MAT_DIELECTRIC;
            const uint32_t ax = v % 3u;
            const float sg = (v / 3u) & 1u ? -1.0f : 1.0f;
            x.entering = (v / 6u) & 1u;
            x.param = x.entering ? ((v / 12u) & 1u ? 0.75f : 0.5f) : iors[1u + (v / 12u) % 3u];
            const float eta = x.entering ? 1.0f / x.param : x.param;
            const float ci = ulps((float)std::sqrt(1.0 - 1.0 / ((double)eta * eta)), (int)((v / 36u) % 33u) - 16);
            x.nf[0] = x.nf[1] = x.nf[2] = 0.0f;
            x.nf[ax] = sg;
            x.d[0] = x.d[1] = x.d[2] = 0.0f;
            x.d[ax] = -ci * sg;
            x.d[(ax + 1u) % 3u] = std::sqrt(1.0f - ci * ci);
            const float s2 = std::fmax(1.0f - ci * ci, 0.0f), kk = (eta * eta) * s2;
            k_one += kk == 1.0f;
            k_near += kk != 1.0f && std::fabs(kk - 1.0f) < 0x1p-20f;
        } else if (mode == 5u) {  // normal incidence
            for (int c = 0; c < 3; ++c) x.d[c] = -x.nf[c];
            ++normal_inc;
        } else if (mode == 6u) {  // METAL(1): the reflected and the fuzz vector cancel (exactly: |r + b|^2 = 0, below
            // inv_sqrt_ref's fast range) or all but cancel. Axis normal: r is d mirrored, exactly
            x.kind = SPT_MAT_METAL;
            const uint32_t ax = v % 3u;
            x.nf[0] = x.nf[1] = x.nf[2] = 0.0f;
            x.nf[ax] = (v / 3u) & 1u ? -1.0f : 1.0f;
            uint32_t s = x.state;
            float b[3];
            ref_bounce_dir(x.nf, &s, x.flags, b);
            for (int c = 0; c < 3; ++c) x.d[c] = (uint32_t)c == ax ? b[c] : -b[c];
            const uint32_t var = (v / 6u) & 3u;
            x.param = var == 2u ? 0x1.fffffep-1f : 1.0f;
            if (var & 1u) x.d[(ax + 1u) % 3u] = ulps(x.d[(ax + 1u) % 3u], var == 1u ? 1 : -1);
        } else if (mode == 7u) {  // ior = 1
            x.kind = SPT_MAT_DIELECTRIC;
            x.param = 1.0f;
            const float dn = (d[0] * x.nf[0] + d[1] * x.nf[1]) + d[2] * x.nf[2];
            for (int c = 0; c < 3; ++c) x.d[c] = dn > 0.0f ? -d[c] : d[c];
        } else {  // any direction arriving against nf
            const float dn = (d[0] * x.nf[0] + d[1] * x.nf[1]) + d[2] * x.nf[2];
            for (int c = 0; c < 3; ++c) x.d[c] = dn > 0.0f ? -d[c] : d[c];
        }
        ior1 += x.kind == SPT_MAT_DIELECTRIC && x.param == 1.0f;
        if (x.kind == SPT_MAT_METAL) ++fuzz[x.param == 0.0f ? 0 : (x.param == 1.0f ? 1 : 2)];
        ++enter[x.entering];
    }
    std::vector<BsdfOut> want(n);
    uint64_t host_bad = 0;
    {
        Clock clk;
        for (uint32_t i = 0; i < n; ++i) {
            const BsdfIn& x = in[i];
            const spt_material_model m{x.kind, x.param, {0, 0}};
            uint32_t s = x.state;
            int tr = 0;
            const int ab = mat_scatter(&m, x.d, x.nf, (int)x.entering, x.flags, &s, want[i].d0, &tr);
            want[i].f0 = (tr ? 1u : 0u) | (ab ? 2u : 0u);
            want[i].s0 = s;
            if (x.kind == SPT_MAT_DIELECTRIC) {
                const float eta = x.entering ? 1.0f / x.param : x.param;
                const float ci = std::fmin(-((x.d[0] * x.nf[0] + x.d[1] * x.nf[1]) + x.d[2] * x.nf[2]), 1.0f);
                tir += (eta * eta) * std::fmax(1.0f - ci * ci, 0.0f) > 1.0f;
                ++(tr ? transmit : reflect);
            }
            absorbed += ab != 0;
            cancel += want[i].d0[0] != want[i].d0[0];
            // the host build (what spt_bsdf_sample calls)
            uint32_t hs = x.state;
            const spt::Scatter sc = spt::bsdf_scatter<false>(x.kind, x.param, F3{x.d[0], x.d[1], x.d[2]},
                                                             F3{x.nf[0], x.nf[1], x.nf[2]}, x.entering != 0u, x.flags, hs);
            const uint32_t hf = (sc.transmitted ? 1u : 0u) | (sc.absorbed ? 2u : 0u);
            if ((!same3(&sc.dir.x, want[i].d0) || hf != want[i].f0 || hs != s) && !host_bad++)
                sec.mismatch("host build, input " + std::to_string(i) + " d " + hex(x.d, 3) + " nf " + hex(x.nf, 3) +
                             " param " + hex(&x.param, 1) + " got " + hex(&sc.dir.x, 3) + " want " + hex(want[i].d0, 3));
        }
    }
    sec.n = n;
    if (!g_host) {
        Dev<BsdfIn> din(in);
        Dev<BsdfOut> out(n);
        k_bsdf<<<grid(n), 256>>>(din.p, n, out.p);
        ran("k_bsdf");
        const std::vector<BsdfOut> got = out.get();
        for (uint32_t i = 0; i < n; ++i) {
            const BsdfOut &g = got[i], &w = want[i];
            if (!same3(g.d0, w.d0) || !same3(g.d1, w.d0) || g.f0 != w.f0 || g.f1 != w.f0 || g.s0 != w.s0 || g.s1 != w.s0) {
                const BsdfIn& x = in[i];
                sec.mismatch("input " + std::to_string(i) + " kind " + std::to_string(x.kind) + " param " + hex(&x.param, 1) +
                             " d " + hex(x.d, 3) + " nf " + hex(x.nf, 3) + " entering " + std::to_string(x.entering) +
                             " flags " + std::to_string(x.flags) + " state " + hexu(x.state) + " <false> " + hex(g.d0, 3) +
                             " f" + std::to_string(g.f0) + " <true> " + hex(g.d1, 3) + " f" + std::to_string(g.f1) +
                             " want " + hex(w.d0, 3) + " f" + std::to_string(w.f0));
            }
        }
    }
    sec.need("tir", tir);
    sec.need("k=1", k_one);
    sec.need("k~1", k_near);
    sec.need("transmit", transmit);
    sec.need("reflect_glass", reflect);
    sec.need("absorbed", absorbed);
    sec.need("exact_cancel", cancel);
    sec.need("ior=1", ior1);
    sec.need("normal_incidence", normal_inc);
    sec.need("grazing", grazing);
    sec.need("entering", enter[1]);
    sec.need("leaving", enter[0]);
    sec.need("fuzz=0", fuzz[0]);
    sec.need("fuzz=1", fuzz[1]);
    sec.need("fuzz_other", fuzz[2]);
    return sec.report();
}

// ======================================================================================================
// 5. light sample
// ======================================================================================================
struct LightIn {
    float x[3], n[3], T[3];
    uint32_t state;
};
struct LightOut {
    float w[3], tmax, add[3];
    uint32_t ret, state;
};
template <bool kSpheres>
__global__ void k_light(const float4* emit, uint32_t n_emit, const LightIn* in, uint32_t n, LightOut* out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const LightIn v = in[i];
    uint32_t s = v.state;
    F3 w{0, 0, 0}, add{0, 0, 0};
    float tmax = 0.0f;
    const bool r = spt::light_sample<kSpheres>(emit, n_emit, F3{v.x[0], v.x[1], v.x[2]}, F3{v.n[0], v.n[1], v.n[2]},
                                               F3{v.T[0], v.T[1], v.T[2]}, s, w, tmax, add);
    out[i] = LightOut{{w.x, w.y, w.z}, tmax, {add.x, add.y, add.z}, r ? 1u : 0u, s};
}

bool check_light() {
    Section sec("light");
    struct Table {
        std::string name;
        std::vector<spt_prim> prims;
        std::vector<spt_material> mats;
        bool spheres;
    };
    std::vector<Table> tables(3);
    {  // Cornell's
        Table& t = tables[0];
        t.name = "cornell";
        uint32_t np = 0, nm = 0;
        spt_env env;
        if (spt_build_scene(SPT_SCENE_CORNELL, nullptr, &np, nullptr, &nm, &env) != SPT_OK) return false;
        t.prims.resize(np);
        t.mats.resize(nm);
        if (spt_build_scene(SPT_SCENE_CORNELL, t.prims.data(), &np, t.mats.data(), &nm, &env) != SPT_OK) return false;
        t.spheres = false;
    }
    auto prim3 = [](uint32_t type, uint32_t mat, const float a[4], const float b[3], const float c[3]) {
        spt_prim p{};
        p.type = type, p.material = mat;
        for (int k = 0; k < 3; ++k) p.p0[k] = a[k], p.p1[k] = b[k], p.p2[k] = c[k];
        p.p0[3] = type == SPT_PRIM_SPHERE ? a[3] : 0.0f;
        return p;
    };
    const float qa[4] = {-1, 3, -1, 0}, qu[3] = {2, 0, 0}, qv[3] = {0, 0, 2};                    // a quad in y = 3
    const float ta[4] = {2, 0.5f, 1, 0}, tb[3] = {3, 1.5f, 1.25f}, tc[3] = {2.5f, 0.25f, 3};    // a tilted triangle
    const float sa[4] = {-2, 1, 2, 0.75f}, z3[3] = {0, 0, 0};                                    // a sphere
    const float fa[4] = {-4, 0, -4, 0}, fu[3] = {8, 0, 0}, fv[3] = {0, 0, 8};                    // a floor (no emission)
    for (int k = 1; k < 3; ++k) {
        Table& t = tables[k];
        t.name = k == 1 ? "quad+triangle+sphere" : "quad+triangle";
        t.mats = {spt_material{{0.7f, 0.7f, 0.7f}, {0, 0, 0}}, spt_material{{0.5f, 0.5f, 0.5f}, {4.0f, 3.0f, 2.0f}},
                  spt_material{{0.5f, 0.5f, 0.5f}, {0.0f, 1.5f, 7.0f}}};
        t.prims = {prim3(SPT_PRIM_QUAD, 0, fa, fu, fv), prim3(SPT_PRIM_QUAD, 1, qa, qu, qv),
                   prim3(SPT_PRIM_TRIANGLE, 2, ta, tb, tc)};
        if (k == 1) t.prims.push_back(prim3(SPT_PRIM_SPHERE, 1, sa, z3, z3));
        t.spheres = k == 1;
    }
    uint64_t ret[2] = {0, 0}, cl0 = 0, behind = 0, in_sphere = 0, out_sphere = 0, kinds[3] = {0, 0, 0}, no_sphere_tables = 0;
    for (Table& t : tables) {
        std::vector<spt::DevEmitter> em;
        spt::build_emitters(t.prims.data(), (uint32_t)t.prims.size(), t.mats.data(), em);
        const spt_env env{};
        ref_scene* rs = ref_scene_create(t.prims.data(), (uint32_t)t.prims.size(), t.mats.data(), (uint32_t)t.mats.size(), &env);
        if (em.empty() || em.size() != ref_emitter_count(rs)) {
            sec.mismatch(t.name + ": " + std::to_string(em.size()) + " emitter records, the oracle has " +
                         std::to_string(ref_emitter_count(rs)));
            ref_scene_destroy(rs);
            continue;
        }
        const uint32_t n = 1u << 16;
        std::vector<LightIn> in(n);
        for (uint32_t i = 0; i < n; ++i) {
            LightIn& v = in[i];
            const uint32_t fam = i & 7u, h = hash32(i * 11u + (uint32_t)t.prims.size());
            v.state = hash32(i * 7u + 5u);
            for (int c = 0; c < 3; ++c) v.T[c] = fam == 7u && c == 1 ? 0.0f : u01(h + 20u + c);
            unit3(i + 0x1000000u, v.n);
            // the emitter this state's first draw picks, to aim the special points at it
            uint32_t s = v.state;
            const float u0 = ref_random_float(&s);
            uint32_t j = (uint32_t)(u0 * (float)em.size());
            j = j < em.size() ? j : (uint32_t)em.size() - 1u;
            const spt::DevEmitter& e = em[j];
            const uint32_t kind = bits(e.base[3]);
            for (int c = 0; c < 3; ++c) v.x[c] = 3.0f * s11(h + c) + (c == 1 ? 1.0f : 0.0f);
            if (kind == 2u && fam < 3u) {  // inside the sphere, and just outside
                float dir[3];
                unit3(h, dir);
                const float f = fam == 0u ? 0.9f * u01(h + 7u) : (fam == 1u ? 1.001f : 0.999f);
                for (int c = 0; c < 3; ++c) v.x[c] = e.base[c] + (e.e1[0] * f) * dir[c];
            } else if (kind != 2u && fam == 0u) {  // in the emitter's plane: base + a e1 + b e2 outside the emitter
                const float a = 2.0f + u01(h + 7u), b = -1.0f - u01(h + 8u);
                for (int c = 0; c < 3; ++c) v.x[c] = (e.base[c] + a * e.e1[c]) + b * e.e2[c];
            }
            if (fam == 3u)  // the shading normal points away from every emitter (they lie above y = 0)
                v.n[0] = 0.0f, v.n[1] = -1.0f, v.n[2] = 0.0f, v.x[1] = -0.5f;
            else if (fam != 6u && v.n[1] < 0.0f)
                v.n[1] = -v.n[1];
        }
        std::vector<LightOut> want(n);
        {
            Clock clk;
            for (uint32_t i = 0; i < n; ++i) {
                LightOut& w = want[i];
                uint32_t s = in[i].state;
                w.tmax = 0.0f, w.add[0] = w.add[1] = w.add[2] = 0.0f;
                w.ret = (uint32_t)ref_light_sample(rs, in[i].x, in[i].n, in[i].T, &s, w.w, &w.tmax, w.add);
                w.state = s;
            }
        }
        for (uint32_t i = 0; i < n; ++i) {  // the counters, from the chosen emitter and the oracle's w
            uint32_t s = in[i].state;
            const float u0 = ref_random_float(&s);
            uint32_t j = (uint32_t)(u0 * (float)em.size());
            j = j < em.size() ? j : (uint32_t)em.size() - 1u;
            const spt::DevEmitter& e = em[j];
            const uint32_t kind = bits(e.base[3]);
            ++kinds[kind < 3u ? kind : 0u];
            ++ret[want[i].ret ? 1 : 0];
            const float* w = want[i].w;
            behind += !((in[i].n[0] * w[0] + in[i].n[1] * w[1]) + in[i].n[2] * w[2] > 0.0f);
            if (kind == 2u) {
                const float xc[3] = {in[i].x[0] - e.base[0], in[i].x[1] - e.base[1], in[i].x[2] - e.base[2]};
                ++(norm2(xc) < e.e1[0] * e.e1[0] ? in_sphere : out_sphere);
            } else {
                cl0 += (e.nl[0] * w[0] + e.nl[1] * w[1]) + e.nl[2] * w[2] == 0.0f;
            }
        }
        sec.n += n;
        no_sphere_tables += !t.spheres;
        if (!g_host) {
            Dev<spt::DevEmitter> dem(em);
            Dev<LightIn> din(in);
            for (int variant = 0; variant < (t.spheres ? 1 : 2); ++variant) {
                Dev<LightOut> out(n);
                if (variant == 0)
                    k_light<true><<<grid(n), 256>>>((const float4*)dem.p, (uint32_t)em.size(), din.p, n, out.p);
                else
                    k_light<false><<<grid(n), 256>>>((const float4*)dem.p, (uint32_t)em.size(), din.p, n, out.p);
                ran("k_light");
                const std::vector<LightOut> got = out.get();
                for (uint32_t i = 0; i < n; ++i) {
                    const LightOut &g = got[i], &w = want[i];
                    bool ok = g.ret == w.ret && g.state == w.state && same3(g.w, w.w);
                    if (ok && w.ret) ok = same(g.tmax, w.tmax) && same3(g.add, w.add);
                    if (!ok)
                        sec.mismatch(t.name + (variant ? " <false>" : " <true>") + " input " + std::to_string(i) + " x " +
                                     hex(in[i].x, 3) + " n " + hex(in[i].n, 3) + " T " + hex(in[i].T, 3) + " state " +
                                     hexu(in[i].state) + " got " + std::to_string(g.ret) + " " + hex(g.w, 7) + " want " +
                                     std::to_string(w.ret) + " " + hex(w.w, 7));
                }
            }
        }
        ref_scene_destroy(rs);
    }
    sec.need("sampled", ret[1]);
    sec.need("rejected", ret[0]);
    sec.need("cl=0", cl0);
    sec.need("behind_normal", behind);
    sec.need("inside_sphere", in_sphere);
    sec.need("outside_sphere", out_sphere);
    sec.need("quad", kinds[0]);
    sec.need("triangle", kinds[1]);
    sec.need("sphere", kinds[2]);
    sec.need("tables_without_spheres", no_sphere_tables);
    return sec.report();
}

// ======================================================================================================
// 6. octa_texel
// ======================================================================================================
struct OctaIn {
    float d[3];
    uint32_t w, h;
};
__global__ void k_octa(const OctaIn* in, uint32_t n, uint32_t* out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[i] = spt::octa_texel(in[i].d[0], in[i].d[1], in[i].d[2], in[i].w, in[i].h);
}

bool check_octa() {
    Section sec("octa");
    std::vector<OctaIn> in;
    const uint32_t sizes[4][2] = {{1, 1}, {3, 5}, {64, 64}, {4096, 4096}};
    uint64_t folds = 0, zero_vec = 0, zero_y = 0, axes = 0, lower = 0;
    for (const auto& sz : sizes) {
        auto add = [&](float x, float y, float z) { in.push_back(OctaIn{{x, y, z}, sz[0], sz[1]}); };
        for (int a = 0; a < 3; ++a)
            for (float s : {1.0f, -1.0f, 0.5f, -3.0f}) {
                float d[3] = {0, 0, 0};
                d[a] = s;
                add(d[0], d[1], d[2]);
                ++axes;
            }
        add(0.0f, 0.0f, 0.0f), add(-0.0f, -0.0f, -0.0f), add(0.0f, -0.0f, 0.0f);
        zero_vec += 3;
        for (uint32_t k = 0; k < 64u; ++k) {  // dy = +-0; the fold diagonals |px| = |pz| in the lower hemisphere
            const float x = s11(k * 3u + 1u), z = s11(k * 3u + 2u);
            add(x, k & 1u ? -0.0f : 0.0f, z);
            ++zero_y;
            for (float y : {-0.5f, -0x1p-30f, 0.25f})
                for (int sg = 0; sg < 4; ++sg)
                    for (int nudge = -1; nudge <= 1; ++nudge) {
                        add(sg & 1 ? -x : x, y, ulps(sg & 2 ? -x : x, nudge));
                        ++folds;
                    }
        }
        for (uint32_t i = 0; i < 20000u; ++i) {
            float d[3];
            unit3(i * 4u + sz[0], d);
            const float scale = i & 1u ? 1.0f : std::ldexp(1.0f, (int)(hash32(i) % 60u) - 30);
            add(d[0] * scale, d[1] * scale, d[2] * scale);
            lower += d[1] < 0.0f;
        }
    }
    const uint32_t n = (uint32_t)in.size();
    std::vector<uint32_t> want(n);
    uint64_t host_bad = 0;
    {
        Clock clk;
        for (uint32_t i = 0; i < n; ++i) {
            want[i] = ref_octa_texel(in[i].d[0], in[i].d[1], in[i].d[2], in[i].w, in[i].h);
            const uint32_t hb = spt::octa_texel(in[i].d[0], in[i].d[1], in[i].d[2], in[i].w, in[i].h);
            if (hb != want[i] && !host_bad++)
                sec.mismatch("host build, d " + hex(in[i].d, 3) + " map " + std::to_string(in[i].w) + "x" +
                             std::to_string(in[i].h) + " got " + std::to_string(hb) + " want " + std::to_string(want[i]));
        }
    }
    for (uint32_t i = 0; i < n; ++i)
        if (in[i].d[0] == 0.0f && in[i].d[1] == 0.0f && in[i].d[2] == 0.0f && want[i] != 0u)
            sec.mismatch("the zero vector maps to texel " + std::to_string(want[i]));
    sec.n = n;
    if (!g_host) {
        Dev<OctaIn> din(in);
        Dev<uint32_t> out(n);
        k_octa<<<grid(n), 256>>>(din.p, n, out.p);
        ran("k_octa");
        const std::vector<uint32_t> got = out.get();
        for (uint32_t i = 0; i < n; ++i)
            if (got[i] != want[i])
                sec.mismatch("d " + hex(in[i].d, 3) + " map " + std::to_string(in[i].w) + "x" + std::to_string(in[i].h) +
                             " got " + std::to_string(got[i]) + " want " + std::to_string(want[i]));
    }
    sec.need("axes", axes);
    sec.need("dy=+-0", zero_y);
    sec.need("fold_diagonals", folds);
    sec.need("zero_vector", zero_vec);
    sec.need("lower_hemisphere", lower);
    return sec.report();
}

}  // namespace

int main(int argc, char** argv) {
    g_host = argc > 1 && std::strcmp(argv[1], "--host") == 0;
    if (argc > 1 && !g_host) {
        std::printf("usage: test_device_rays [--host]\n");
        return 1;
    }
    const auto t0 = std::chrono::steady_clock::now();
    bool ok = true;
    try {
        ok = check_camera() && ok;
        ok = check_intersectors() && ok;
        ok = check_sincos() && ok;
        ok = check_bounce() && ok;
        ok = check_bsdf() && ok;
        ok = check_light() && ok;
        ok = check_octa() && ok;
    } catch (const HipFail&) {
        return 2;
    }
    std::printf("%s: expected values %.2f s, total %.2f s\n", g_host ? "host only (no kernel launched)" : "device",
                g_oracle_s, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    std::printf(ok ? "PASS\n" : "FAIL\n");
    return ok ? 0 : 1;
}
