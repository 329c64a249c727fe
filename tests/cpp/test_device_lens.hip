// Ray-level GPU check of spt_device.h camera_lens_ray (the thin lens): the device build, both sincos forms,
// against the host build (sqrtf and '/'; the same FMA sequence in sincos_2pi), origin and direction bit for
// bit, in the way test_device_rays.hip checks camera_ray_dir. Inputs: a grid of pixels, jitter and aperture
// samples (u1, u2) with their endpoints (u1 = +0, 2^-32, 1, values below sqrt_unit's range, and +inf, NaN,
// a negative value and -0 past its other end; u2 = 0, the quarter turns, 1), on cameras and lenses placed on
// either side of every term of the device fast path's gates: u1 against 2^-96, q = |t|^2 against 2^-80 and 2^40, the numerators against 2^-100 and 2^50, zero
// numerators, quotients that tie between two denormals and roots decided by a zero residual.
// `--host` launches nothing: it builds the same inputs and asserts that every branch they are aimed at is
// reached (the coverage counters, also asserted in a GPU run). One line: inputs, mismatches, the first
// mismatching input in hex, the counters. PASS / FAIL, exit status 0 / 1; 2 on a HIP error (nothing is
// launched after one).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "spt_device.h"

using spt::CameraLens;
using spt::CameraPose;
using spt::F3;

namespace {

struct HipFail {};
bool g_host = false;

void ck(hipError_t e, const char* what) {
    if (e == hipSuccess) return;
    std::printf("HIP error: %s: %s\n", what, hipGetErrorString(e));
    throw HipFail{};
}
template <class T>
struct Dev {
    T* p = nullptr;
    size_t n;
    explicit Dev(size_t n_) : n(n_) { ck(hipMalloc((void**)&p, (n ? n : 1) * sizeof(T)), "hipMalloc"); }
    Dev(const Dev&) = delete;
    ~Dev() { (void)hipFree(p); }
    std::vector<T> get() const {
        std::vector<T> v(n);
        if (n) ck(hipMemcpy(v.data(), p, n * sizeof(T), hipMemcpyDeviceToHost), "hipMemcpy to host");
        return v;
    }
};
inline uint32_t grid(size_t n) { return (uint32_t)((n + 255u) / 256u); }

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
inline float ulps(float x, int k) {
    int64_t i = bits(x);
    if (i & 0x80000000ll) i = -(i & 0x7fffffffll) - 1;
    i += k;
    return fbits(i < 0 ? (uint32_t)(-(i + 1)) | 0x80000000u : (uint32_t)i);
}
inline bool same(float a, float b) { return bits(a) == bits(b) || (a != a && b != b); }
inline bool same3(const F3& a, const F3& b) { return same(a.x, b.x) && same(a.y, b.y) && same(a.z, b.z); }
inline float u01(uint32_t h) { return (float)(hash32(h) >> 8) * 0x1p-24f; }
inline float s11(uint32_t h) { return u01(h) * 2.0f - 1.0f; }
inline float norm2(const float v[3]) { return (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]; }
// a vector with no small component whose computed (x*x + y*y) + z*z is exactly `target`
bool find_norm2(float target, uint32_t seed, float v[3]) {
    for (uint32_t tries = 0; tries < 100000u; ++tries) {
        const uint32_t h = seed * 100003u + tries;
        const double x = s11(h * 3u + 0x1111u), y = s11(h * 3u + 0x2222u), z = s11(h * 3u + 0x3333u);
        const double l = std::sqrt(x * x + y * y + z * z);
        if (!(l > 0.05)) continue;
        float u[3] = {(float)(x / l), (float)(y / l), (float)(z / l)};
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

// input i of a case: jitter and the aperture sample, endpoints and hashed values
struct Sample {
    float jx, jy, u1, u2;
};
__host__ __device__ inline Sample sample_of(uint32_t i, uint32_t seed) {
    const uint32_t h = hash32(i * 2u + seed);
    Sample s;
    const uint32_t jm = h & 3u, m1 = ((h >> 2) & 15u) % 12u, m2 = (h >> 6) & 7u;
    s.jx = s.jy = jm == 0u ? 0.0f : (jm == 1u ? 0x1.fffffep-1f : 1.0f);
    if (jm >= 2u) {
        s.jx = (float)(hash32(h) >> 8) * 0x1p-24f;
        s.jy = (float)(hash32(h ^ 0x9e3779b9u) >> 8) * 0x1p-24f;
    }
    const float r1 = (float)(hash32(h ^ 0x51ed270bu) >> 8) * 0x1p-24f;
    const float r2 = (float)(hash32(h ^ 0x2545f491u) >> 8) * 0x1p-24f;
    // u1: +0, random_float's smallest non-zero value and its 1.0f; below sqrt_unit's range (2^-97, 2^-96
    // itself, a denormal); hashed; and what no random_float gives but the function is defined for, past
    // the gate's other end: +inf, a NaN, a negative value, -0 (the general sqrtf)
    const float u1s[12] = {0.0f, 0x1p-32f, 1.0f, 0x1p-97f, 0x1p-96f, 0x1p-140f, r1, r1 * r1,
                           __builtin_inff(), __builtin_nanf(""), -0.25f, -0.0f};
    // u2: the quarter turns (phi a multiple of pi / 2 in fp32), the ends, hashed
    const float u2s[8] = {0.0f, 0.25f, 0.5f, 0.75f, 1.0f, 0x1p-32f, r2, r2};
    s.u1 = u1s[m1];
    s.u2 = u2s[m2];
    return s;
}

struct Ray {
    F3 o, d;
};
template <bool kSmem>
__global__ void k_lens(CameraPose c, CameraLens l, uint32_t w, uint32_t row_step, uint32_t n, float inv_w, float inv_h,
                       float aspect, uint32_t seed, Ray* out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const Sample s = sample_of(i, seed);
    Ray r;
    r.d = spt::camera_lens_ray<kSmem>(c, l, i % w, (i / w) * row_step, s.jx, s.jy, s.u1, s.u2, inv_w, inv_h, aspect, r.o);
    out[i] = r;
}

struct Case {
    std::string name;
    CameraPose c;
    CameraLens l;
    bool wide;  // also the 2^20 x 1 image
};
CameraPose pose(const float u[3], const float v[3], const float w[3]) {
    return CameraPose{F3{0.25f, 1.0f, -2.0f}, F3{u[0], u[1], u[2]}, F3{v[0], v[1], v[2]}, F3{w[0], w[1], w[2]}};
}
CameraPose scaled_identity(float su, float sv, float sw) {
    const float u[3] = {su, 0, 0}, v[3] = {0, sv, 0}, w[3] = {0, 0, sw};
    return pose(u, v, w);
}
// spt_camera_look_at's construction (double, rounded once)
CameraPose look(double fx, double fy, double fz, double ux, double uy, double uz, double h) {
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

bool check_lens() {
    std::vector<Case> cases;
    const CameraLens none{0.0f, 0.0f, 1.0f};  // a = b = 0, f = 1: off = 0 and t = p exactly
    cases.push_back({"identity", scaled_identity(1, 1, 1), CameraLens{0.1f, 0.1f, 6.0f}, false});
    cases.push_back({"look_at", look(0.3, -0.4, 0.8, 0.1, 1.0, 0.05, 0.7), CameraLens{0.14f, 0.14f, 6.0f}, false});
    cases.push_back({"wide aperture", look(-1.5, -1.75, 7.0, 0, 1, 0, 0.52), CameraLens{0.96f, 0.96f, 2.5f}, false});
    cases.push_back({"far focus", look(-1.5, -1.75, 7.0, 0, 1, 0, 0.52), CameraLens{0.04f, 0.04f, 40.0f}, false});
    cases.push_back({"a != b", scaled_identity(0.5f, 2.0f, 1), CameraLens{0.2f, 0.05f, 3.0f}, false});
    // straight down each axis without an offset: zero numerators (the general division keeps their sign)
    cases.push_back({"+x", look(1, 0, 0, 0, 1, 0, 1), none, false});
    cases.push_back({"-y", look(0, -1, 0, 0, 0, 1, 1), none, false});
    cases.push_back({"+z f=3", look(0, 0, 1, 0, 1, 0, 1), CameraLens{0.0f, 0.0f, 3.0f}, false});
    cases.push_back({"u=0", scaled_identity(0, 1, 1), CameraLens{0.5f, 0.5f, 2.0f}, false});
    // q = |t|^2 on either side of 2^-80 and of 2^40 (the focus distance scales t: q ~ f^2 (sx^2 + sy^2 + 1))
    cases.push_back({"f=2^-40", scaled_identity(1, 1, 1), CameraLens{0x1p-46f, 0x1p-46f, 0x1p-40f}, false});
    cases.push_back({"f<2^-40", scaled_identity(1, 1, 1), CameraLens{0x1p-46f, 0x1p-46f, 0x1.fffp-41f}, false});
    cases.push_back({"f=2^-43", scaled_identity(1, 1, 1), CameraLens{0x1p-48f, 0x1p-48f, 0x1p-43f}, false});
    cases.push_back({"f<2^20", scaled_identity(1, 1, 1), CameraLens{0.1f, 0.1f, 0x1.6p19f}, false});
    cases.push_back({"f=2^20", scaled_identity(0x1p-30f, 0x1p-30f, 1), CameraLens{0.1f, 0.1f, 0x1p20f}, false});
    cases.push_back({"f<2^20 w", scaled_identity(0x1p-30f, 0x1p-30f, 1), CameraLens{0.0f, 0.0f, 0x1.fffffep19f}, false});
    // ... and the aperture's offset alone past 2^40 (a radius of 2^21 on unit axes)
    cases.push_back({"a=2^21", scaled_identity(1, 1, 1), CameraLens{0x1p21f, 0x1p21f, 1.0f}, false});
    // numerators on either side of 2^-100 (t.x = sx * u.x) and of 2^50
    cases.push_back({"u=2^-100", scaled_identity(0x1p-100f, 1, 1), none, false});
    cases.push_back({"u=2^-103", scaled_identity(0x1p-103f, 0x1p-101f, 1), none, false});
    cases.push_back({"u=2^-100 lens", scaled_identity(0x1p-100f, 1, 1), CameraLens{0.25f, 0.25f, 2.0f}, false});
    cases.push_back({"u=2^50", scaled_identity(0x1p50f, 1, 1), none, false});
    cases.push_back({"u=2^49", scaled_identity(0x1p49f, 0x1p48f, 0x1p30f), none, false});
    // past the gate, q in [2^40, 2^60), where the unscaled division is wrong: len = 1.5 * 2^29 and, in a
    // 2^20 x 1 image without jitter, t.x = 15 m 2^-122 for integers m: for odd m the quotient lies exactly
    // half way between two denormals (test_device_rays.hip "ties")
    cases.push_back({"ties", scaled_identity(0x1.ep-120f, 1, 0x1.8p29f), none, true});
    // q next to an even power of two: sqrtf's result is decided by a residual that is exactly zero
    const float targets[4] = {0x1.fffffep-1f, 0x1.000002p0f, 0x1.fffffep1f, 0x1.000002p2f};
    uint64_t root_ties = 0;
    for (uint32_t k = 0; k < 8u; ++k) {
        float w[3];
        if (!find_norm2(targets[k & 3u], 77u + k, w)) continue;
        const float u[3] = {0x1p-60f, 0, 0}, v[3] = {0, 0x1p-60f, 0};
        cases.push_back({"q~2^k", pose(u, v, w), none, false});
        ++root_ties;
    }
    const uint32_t sizes[3][3] = {{37, 23, 1}, {1920, 1080, 47}, {1u << 20, 1, 1}};  // w, h, every n-th row

    uint64_t n_in = 0, bad = 0;
    std::string first;
    uint64_t fast = 0, general = 0, q_lo[2] = {0, 0}, q_hi[2] = {0, 0}, n_lo[2] = {0, 0}, n_hi[2] = {0, 0};
    uint64_t zero_num = 0, u1_unit = 0, u1_general = 0, u1_below = 0, u1_inf = 0, u1_nan = 0, u1_neg = 0, u1_negzero = 0, u1_zero = 0, u1_one = 0, u2_one = 0, quarter = 0, moved = 0;
    std::vector<Ray> want;
    for (size_t ci = 0; ci < cases.size(); ++ci) {
        const CameraPose& c = cases[ci].c;
        const CameraLens& l = cases[ci].l;
        for (const auto& sz : sizes) {
            const uint32_t w = sz[0], h = sz[1], step = sz[2], rows = (h + step - 1u) / step, n = w * rows;
            if (w == (1u << 20) && !cases[ci].wide) continue;
            const float inv_w = 1.0f / (float)w, inv_h = 1.0f / (float)h, aspect = (float)w / (float)h;
            const uint32_t seed = (uint32_t)ci * 977u + w;
            want.resize(n);
            for (uint32_t i = 0; i < n; ++i) {
                const Sample s = sample_of(i, seed);
                const uint32_t x = i % w, y = (i / w) * step;
                want[i].d = spt::camera_lens_ray(c, l, x, y, s.jx, s.jy, s.u1, s.u2, inv_w, inv_h, aspect, want[i].o);
                // the gates' terms, restated for the counters only
                const bool unit = bits(s.u1) == 0u || (s.u1 >= 0x1p-96f && s.u1 < INFINITY);
                ++(unit ? u1_unit : u1_general);
                u1_below += s.u1 > 0.0f && s.u1 < 0x1p-96f;
                u1_inf += s.u1 == INFINITY;
                u1_nan += s.u1 != s.u1;
                u1_neg += s.u1 < 0.0f;
                u1_negzero += bits(s.u1) == 0x80000000u;
                u1_zero += s.u1 == 0.0f;
                u1_one += s.u1 == 1.0f;
                u2_one += s.u2 == 1.0f;
                quarter += s.u2 == 0.25f || s.u2 == 0.5f || s.u2 == 0.75f;
                const float px = (float)x + s.jx, py = (float)y + s.jy;
                const float sx = ((px * inv_w) * 2.0f - 1.0f) * aspect, sy = (1.0f - py * inv_h) * 2.0f - 1.0f;
                const float p[3] = {(sx * c.u.x + sy * c.v.x) + c.w.x, (sx * c.u.y + sy * c.v.y) + c.w.y,
                                    (sx * c.u.z + sy * c.v.z) + c.w.z};
                const float off[3] = {want[i].o.x - c.o.x, want[i].o.y - c.o.y, want[i].o.z - c.o.z};
                moved += off[0] != 0.0f || off[1] != 0.0f || off[2] != 0.0f;
                // (t from the origin the function returned: exact where the offset is zero, the cases the
                // numerator and root-tie counters are aimed at; elsewhere a close restatement)
                const float t[3] = {l.f * p[0] - off[0], l.f * p[1] - off[1], l.f * p[2] - off[2]};
                const float q = norm2(t);
                bool lo = true, hi = true;
                for (float a : t) {
                    lo = lo && std::fabs(a) >= 0x1p-100f;
                    hi = hi && std::fabs(a) <= 0x1p50f;
                    zero_num += a == 0.0f;
                }
                ++q_lo[q >= 0x1p-80f], ++q_hi[q < 0x1p40f], ++n_lo[lo], ++n_hi[hi];
                ++((q >= 0x1p-80f && q < 0x1p40f && lo && hi) ? fast : general);
            }
            n_in += n;
            if (g_host) continue;
            for (int form = 0; form < 2; ++form) {
                Dev<Ray> out(n);
                if (form == 0) k_lens<false><<<grid(n), 256>>>(c, l, w, step, n, inv_w, inv_h, aspect, seed, out.p);
                else k_lens<true><<<grid(n), 256>>>(c, l, w, step, n, inv_w, inv_h, aspect, seed, out.p);
                ck(hipGetLastError(), "k_lens");
                ck(hipDeviceSynchronize(), "k_lens");
                const std::vector<Ray> got = out.get();
                for (uint32_t i = 0; i < n; ++i)
                    if (!same3(got[i].o, want[i].o) || !same3(got[i].d, want[i].d)) {
                        const Sample s = sample_of(i, seed);
                        const float in[4] = {s.jx, s.jy, s.u1, s.u2};
                        if (!bad++)
                            first = "lens " + cases[ci].name + " sincos form " + std::to_string(form) + " " +
                                    std::to_string(w) + "x" + std::to_string(h) + " pixel " + std::to_string(i % w) + "," +
                                    std::to_string((i / w) * step) + " jx jy u1 u2 " + hex(in, 4) + " got o " +
                                    hex(&got[i].o.x, 3) + " d " + hex(&got[i].d.x, 3) + " want o " + hex(&want[i].o.x, 3) +
                                    " d " + hex(&want[i].d.x, 3);
                    }
            }
        }
    }
    const std::pair<const char*, uint64_t> cover[] = {
        {"fast", fast}, {"general", general}, {"q<2^-80", q_lo[0]}, {"q>=2^-80", q_lo[1]}, {"q>=2^40", q_hi[0]},
        {"q<2^40", q_hi[1]}, {"num<2^-100", n_lo[0]}, {"num>=2^-100", n_lo[1]}, {"num>2^50", n_hi[0]},
        {"num<=2^50", n_hi[1]}, {"zero_num", zero_num}, {"u1_sqrt_unit", u1_unit}, {"u1_general", u1_general}, {"u1<2^-96", u1_below}, {"u1=inf", u1_inf},
        {"u1=nan", u1_nan}, {"u1<0", u1_neg}, {"u1=-0", u1_negzero},
        {"u1=0", u1_zero}, {"u1=1", u1_one}, {"u2=1", u2_one}, {"quarter_turns", quarter}, {"origin_moved", moved},
        {"root_tie_cameras", root_ties}};
    bool cover_ok = true;
    std::printf("lens: %llu inputs%s, %llu mismatches%s%s;", (unsigned long long)n_in, g_host ? " (host: not launched)" : " x 2 forms",
                (unsigned long long)bad, bad ? ", first: " : "", first.c_str());
    for (const auto& c : cover) {
        std::printf(" %s=%llu", c.first, (unsigned long long)c.second);
        cover_ok = cover_ok && c.second != 0u;
    }
    std::printf("%s\n", cover_ok ? "" : "  [a branch is not reached]");
    return bad == 0 && cover_ok;
}

}  // namespace

int main(int argc, char** argv) {
    g_host = argc > 1 && std::strcmp(argv[1], "--host") == 0;
    if (argc > 1 && !g_host) {
        std::printf("usage: test_device_lens [--host]\n");
        return 2;
    }
    bool ok = false;
    try {
        ok = check_lens();
    } catch (const HipFail&) {
        return 2;
    }
    std::puts(ok ? "PASS" : "FAIL");
    return ok ? 0 : 1;
}
