// spt_device.h — device-side arithmetic of the integrator (gfx950).
//
// Every function restates one piece of render::CPUPathTracer
// (libs/render/src/engines/pathtracer/backends/cpu/CPUPathTracer.cpp) with the exact float
// evaluation order of the reference's Linux build (SURVEY.md §8a "numeric semantics"):
//   - no FMA contraction (the whole library is compiled with -ffp-contract=off),
//   - correctly rounded fp32 '/' and sqrtf (HIP default),
//   - glm formulas: dot = (x*x' + y*y') + z*z', cross = (a.y*b.z - b.y*a.z, ...),
//     normalize(v) = v * (1.0f / sqrtf(dot(v, v))), mix(x, y, a) = x*(1-a) + y*a,
//   - get_random_bounche's unqualified sqrt/cos/sin on float arguments bind to the C double
//     functions under libstdc++, so cos/sin and the products with sinTheta run in fp64.
// oracle/cpu_ref.c restates the same functions on the CPU; tests compare the two bit for bit.
#pragma once

#ifndef __HIPCC_RTC__
#include <hip/hip_runtime.h>
#include <stdint.h>
#else  // hiprtc (spt_jit.cpp): no system headers; its runtime header defines the fixed-width types
typedef __hip_internal::uint8_t uint8_t;
typedef __hip_internal::uint16_t uint16_t;
typedef __hip_internal::uint32_t uint32_t;
typedef __hip_internal::uint64_t uint64_t;
typedef __hip_internal::int32_t int32_t;
#endif

namespace spt {

constexpr float kInf = __builtin_inff();
constexpr uint32_t kMiss = 0xffffffffu;        // RTC_INVALID_GEOMETRY_ID analogue
constexpr float kTNear = 0.001f;               // rayhit.ray.tnear, CPUPathTracer.cpp:221
constexpr float kOriginEps = 1e-4f;            // EPSILON, CPUPathTracer.cpp:277
constexpr float kPiF = 3.14159265358979323846f;  // glm::pi<float>()
constexpr uint32_t kSeedPrime = 982451653u;    // CPUPathTracer.cpp:194
constexpr uint32_t kFlagAbsFloat = 1u;         // SPT_FLAG_ABS_FLOAT

struct F3 {
    float x, y, z;
};

__host__ __device__ __forceinline__ float dot3(F3 a, F3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__host__ __device__ __forceinline__ F3 cross3(F3 a, F3 b) {
    return F3{a.y * b.z - b.y * a.z, a.z * b.x - b.z * a.x, a.x * b.y - b.x * a.y};
}
__host__ __device__ __forceinline__ float sqrt_unit(float x);

// 1.0f / sqrtf(x) as glm::normalize computes it (two correctly rounded operations), bit for bit.
// For x in [2^-96, 2^96) it runs hipcc's own instruction sequences minus the steps that are the
// identity there: sqrtf without its rescaling of x < 2^-96 and its 0/inf pass-through (sqrt_unit),
// and the division 1.0f / s (s in [2^-48, 2^48]) without v_div_scale (no scaling at these
// exponents), the multiply by 1.0 and v_div_fixup (finite, normal quotient). Other x take the
// general routines. 11 VALU operations fewer per call; tests/cpp/test_device_math.hip checks all
// 2^32 inputs against 1.0f / sqrtf(x). SPT_EXPERIMENT_FAST_NORM (measurement-only builds, NOT
// reference numerics: SPT_EXPERIMENT_BUILD must be set too) prices the whole thing with the hardware rsq.
#if (defined(SPT_EXPERIMENT_FAST_NORM) || defined(SPT_EXPERIMENT_FP32_TRIG)) && !defined(SPT_EXPERIMENT_BUILD)
#error "SPT_EXPERIMENT_* flags break parity with the reference: measurement builds only (scripts/build_variant.sh sets SPT_EXPERIMENT_BUILD)"
#endif
// (the host build — spt_bsdf_sample — is the definition itself: 1.0f / sqrtf(x))
__host__ __device__ __forceinline__ float inv_sqrt_ref(float x) {
#ifndef __HIP_DEVICE_COMPILE__
    return 1.0f / sqrtf(x);
#elif defined(SPT_EXPERIMENT_FAST_NORM)
    return __builtin_amdgcn_rsqf(x);
#else
    if (__float_as_uint(x) - 0x0f800000u < 0x60000000u - 0x0f800000u) {  // 2^-96 <= x < 2^96
        const float s = sqrt_unit(x);
        const float y0 = __builtin_amdgcn_rcpf(s);
        const float e = __builtin_fmaf(-s, y0, 1.0f);
        const float y1 = __builtin_fmaf(e, y0, y0);  // q0 = 1.0f * y1
        const float r0 = __builtin_fmaf(-s, y1, 1.0f);
        const float q1 = __builtin_fmaf(r0, y1, y1);
        const float r1 = __builtin_fmaf(-s, q1, 1.0f);
        return __builtin_fmaf(r1, y1, q1);  // v_div_fmas without scaling
    }
    return 1.0f / sqrtf(x);
#endif
}
__host__ __device__ __forceinline__ F3 normalize3(F3 v) {
    const float inv = inv_sqrt_ref(dot3(v, v));
    return F3{v.x * inv, v.y * inv, v.z * inv};
}
// inv_sqrt_ref for an x the CALLER knows to lie in [2^-96, 2^96): the same sequence without the window test
// (the compare and its exec-mask branch). Only for the k_paths step loop of a scene that passed flat_ranges_ok
// (scene.h; spt_kernels.h flat_ranges_baked); each call site states why its x is inside. Same bits there:
// tests/cpp/test_device_ranges.hip compares it with 1.0f / sqrtf(x) over the whole window.
__host__ __device__ __forceinline__ float inv_sqrt_ranged(float x) {
#if !defined(__HIP_DEVICE_COMPILE__) || defined(SPT_EXPERIMENT_FAST_NORM)
    return inv_sqrt_ref(x);
#else
    const float s = sqrt_unit(x);
    const float y0 = __builtin_amdgcn_rcpf(s);
    const float e = __builtin_fmaf(-s, y0, 1.0f);
    const float y1 = __builtin_fmaf(e, y0, y0);
    const float r0 = __builtin_fmaf(-s, y1, 1.0f);
    const float q1 = __builtin_fmaf(r0, y1, y1);
    const float r1 = __builtin_fmaf(-s, q1, 1.0f);
    return __builtin_fmaf(r1, y1, q1);
#endif
}

// get_rng_state, CPUPathTracer.cpp:192-195 (frame = m_frameCount + 1 at the call site :61).
__device__ __forceinline__ uint32_t rng_seed(uint32_t x, uint32_t y, uint32_t width, uint32_t frame1) {
    return x + y * width + frame1 * kSeedPrime;
}

// random_float, CPUPathTracer.cpp:294-301. 4294967295.0f rounds to 2^32, so this is exact.
__host__ __device__ __forceinline__ float random_float(uint32_t& state) {
    state = state * 747796405u + 2891336453u;
    uint32_t r = ((state >> ((state >> 28) + 4u)) ^ state) * 277803737u;
    r = (r >> 22) ^ r;
    return (float)r / 4294967295.0f;
}

// ---- unscaled correctly rounded division (the flat closest-hit loop's fast path) -------------
// hipcc's fp32 n / s is v_div_scale (x2), the reciprocal refinement, the residual steps,
// v_div_fmas and v_div_fixup. For |s| in [2^-40, 2^20] and |n| in [2^-100, 2^50] the scale steps
// are the identity (reciprocal and quotient normal, exponent difference < 96, numerator exponent
// > 23), v_div_fmas is a plain fma and v_div_fixup passes the finite quotient through, so the
// sequence below returns the same bits. For |n| < 2^-100 (zero included) it returns some
// |q| < 2^-59, and so is the exact quotient: every caller rejects both (t < kTNear).
// tests/cpp/test_device_math.hip compares it with n / s on the GPU.
struct RcpRef {
    float s, y;  // the divisor and its refined reciprocal
};
__device__ __forceinline__ RcpRef rcp_ref(float s) {
    const float y0 = __builtin_amdgcn_rcpf(s);
    const float e = __builtin_fmaf(-s, y0, 1.0f);
    return RcpRef{s, __builtin_fmaf(e, y0, y0)};
}
__device__ __forceinline__ float div_ref(float n, RcpRef r) {
    const float q0 = n * r.y;
    const float r0 = __builtin_fmaf(-r.s, q0, n);
    const float q1 = __builtin_fmaf(r0, r.y, q0);
    const float r1 = __builtin_fmaf(-r.s, q1, n);
    return __builtin_fmaf(r1, r.y, q1);
}

// 1.0f / s, correctly rounded: for 2^-40 <= |s| < 2^20 one refined reciprocal and div_ref (the
// numerator 1 is in its range), else hipcc's division. Same bits (tests/cpp/test_device_math.hip checks
// every float); 5 VALU and no v_div_scale / v_div_fixup where the range holds. The BVH triangle test's
// 1 / det and the traversal's inverse direction (trav_init).
__device__ __forceinline__ float recip_ref(float s) {
    const uint32_t a = __float_as_uint(s) & 0x7fffffffu;
    if (a - 0x2b800000u < 0x49800000u - 0x2b800000u) return div_ref(1.0f, rcp_ref(s));  // [2^-40, 2^20)
    return 1.0f / s;
}

// Primary ray, CPUPathTracer.cpp:53-73: pinhole at the origin looking down +z. The fast path's gate
// q = uv_x^2 + uv_y^2 + 1 < 2^40 keeps `len` in [1, 2^20], inside div_ref's divisor range [2^-40, 2^20],
// and the numerators are 0, +-1 or in [2^-100, 2^50] in magnitude (checked per lane): then sqrt_unit
// and one refined reciprocal with div_ref give the correctly rounded sqrtf and quotients. Every real
// image passes (|uv_y| <= 1, |uv_x| <= the aspect ratio < 2^19); a lane outside takes the general
// routines. Same bits. Every k_frame and
// wavefront path pays it once (k_paths once per pixel and launch).
__device__ __forceinline__ F3 primary_dir(uint32_t x, uint32_t y, float inv_w, float inv_h, float aspect) {
    const float u = (float)x * inv_w;
    const float v = 1.0f - (float)y * inv_h;
    const float uv_x = (u * 2.0f - 1.0f) * aspect;
    const float uv_y = v * 2.0f - 1.0f;
    const float q = uv_x * uv_x + uv_y * uv_y + 1.0f;
    auto in_range = [](float c) {  // c == +-0, or 2^-100 <= |c| <= 2^50 (on the magnitude's bits)
        const uint32_t a = __float_as_uint(c) & 0x7fffffffu;
        return (a == 0u) | (a - 0x0d800000u <= 0x58800000u - 0x0d800000u);
    };
    if (((q < 0x1p40f) & in_range(uv_x) & in_range(uv_y))) {
        const RcpRef r = rcp_ref(sqrt_unit(q));
        return F3{div_ref(uv_x, r), div_ref(uv_y, r), div_ref(1.0f, r)};
    }
    const float len = sqrtf(q);
    return F3{uv_x / len, uv_y / len, 1.0f / len};
}

// A posed camera (spt_set_camera, spt.h spt_camera): origin o, image-plane right u and up v (both
// scaled by tan(vfov / 2)) and forward w. The superset of the pinhole above (the reference's Camera.h
// is dead code): u = (1,0,0), v = (0,1,0), w = (0,0,1) at the origin gives primary_dir's bits wherever
// no direction component is zero.
struct CameraPose {
    F3 o, u, v, w;
};

// The camera ray through the point (x + jx, y + jy) of the image plane, y the full-image row; the
// pixel's footprint is [x, x + 1] x [y, y + 1] (jx = jy = 0: its corner, as primary_dir). fp32, no
// contraction, correctly rounded sqrtf and '/': DESIGN.md "Camera" states the expressions, and the
// host (spt_camera_ray) and every kernel compile this one function. On the device a lane whose
// operands are inside sqrt_unit's and div_ref's ranges (q in [2^-80, 2^40), so len in [2^-40, 2^20);
// every numerator in [2^-100, 2^50] in magnitude — a zero one takes the general division, which keeps
// its sign) runs those forms: the same bits (tests/cpp/test_device_rays.hip compares the device build
// with the host's on cameras placed on either side of every term of the gate).
__host__ __device__ inline F3 camera_ray_dir(const CameraPose& c, uint32_t x, uint32_t y, float jx, float jy,
                                             float inv_w, float inv_h, float aspect) {
    const float px = (float)x + jx;
    const float py = (float)y + jy;
    const float u = px * inv_w;
    const float v = 1.0f - py * inv_h;
    const float sx = (u * 2.0f - 1.0f) * aspect;
    const float sy = v * 2.0f - 1.0f;
    const F3 p{(sx * c.u.x + sy * c.v.x) + c.w.x, (sx * c.u.y + sy * c.v.y) + c.w.y, (sx * c.u.z + sy * c.v.z) + c.w.z};
    const float q = (p.x * p.x + p.y * p.y) + p.z * p.z;
#ifdef __HIP_DEVICE_COMPILE__
    auto in_range = [](float a) {  // 2^-100 <= |a| <= 2^50 (on the magnitude's bits)
        return (uint32_t)((__float_as_uint(a) & 0x7fffffffu) - 0x0d800000u <= 0x58800000u - 0x0d800000u);
    };
    // (combined without short-circuits: one branch)
    if (((uint32_t)(q >= 0x1p-80f) & (uint32_t)(q < 0x1p40f) & in_range(p.x) & in_range(p.y) & in_range(p.z))) {
        const RcpRef r = rcp_ref(sqrt_unit(q));
        return F3{div_ref(p.x, r), div_ref(p.y, r), div_ref(p.z, r)};
    }
#endif
    const float len = sqrtf(q);
    return F3{p.x / len, p.y / len, p.z / len};
}

// A thin lens on a posed camera (spt_set_camera_lens): a = radius / |u|, b = radius / |v| (the host's,
// in double, rounded once) turn the camera's tan-scaled u and v into the aperture's axes, and f is the
// focus distance: the points o + f * p, p the un-normalized image-plane vector of camera_ray_dir, are
// in focus.
struct CameraLens {
    float a, b, f;
};
template <bool kSmemCoef>
__host__ __device__ inline void sincos_2pi(double phi, double& s, double& c);

// The lens form of camera_ray_dir: the ray from the point (u1, u2) of the aperture — a uniform point of
// the disc, r = sqrtf(u1), phi = 2 pi u2 as bounce_dir_frame draws its direction — through the point of
// the focus plane the pinhole ray of (x + jx, y + jy) meets. `o` receives the origin, the direction is
// returned. fp32, no contraction, correctly rounded sqrtf and '/', sin and cos by sincos_2pi: DESIGN.md
// "Thin lens" states the expressions, and the host (spt_camera_lens_ray) and every kernel compile this
// one function. On the device u1 = +0 or in [2^-96, inf) takes sqrt_unit (every random_float does), and
// the normalization takes sqrt_unit / div_ref under camera_ray_dir's gate (q in [2^-80, 2^40), every
// numerator in [2^-100, 2^50] in magnitude); other lanes take the general routines. The same bits
// (tests/cpp/test_device_lens.hip compares the device build with the host's on either side of every
// term of both gates).
template <bool kSmemCoef = false>
__host__ __device__ inline F3 camera_lens_ray(const CameraPose& c, CameraLens l, uint32_t x, uint32_t y, float jx,
                                              float jy, float u1, float u2, float inv_w, float inv_h, float aspect,
                                              F3& o) {
    const float px = (float)x + jx;
    const float py = (float)y + jy;
    const float u = px * inv_w;
    const float v = 1.0f - py * inv_h;
    const float sx = (u * 2.0f - 1.0f) * aspect;
    const float sy = v * 2.0f - 1.0f;
    const F3 p{(sx * c.u.x + sy * c.v.x) + c.w.x, (sx * c.u.y + sy * c.v.y) + c.w.y, (sx * c.u.z + sy * c.v.z) + c.w.z};
    float r;
#ifdef __HIP_DEVICE_COMPILE__
    if ((uint32_t)(__float_as_uint(u1) == 0u) | (uint32_t)(__float_as_uint(u1) - 0x0f800000u < 0x7f800000u - 0x0f800000u))
        r = sqrt_unit(u1);
    else
#endif
        r = sqrtf(u1);
    const float phi = 2.0f * kPiF * u2;
    double sp, cp;
    sincos_2pi<kSmemCoef>((double)phi, sp, cp);
    const float lx = (float)((double)r * cp);
    const float ly = (float)((double)r * sp);
    const float ax = lx * l.a;
    const float ay = ly * l.b;
    const F3 off{ax * c.u.x + ay * c.v.x, ax * c.u.y + ay * c.v.y, ax * c.u.z + ay * c.v.z};
    o = F3{c.o.x + off.x, c.o.y + off.y, c.o.z + off.z};
    const F3 t{l.f * p.x - off.x, l.f * p.y - off.y, l.f * p.z - off.z};  // (o + f p) - (o + off)
    const float q = (t.x * t.x + t.y * t.y) + t.z * t.z;
#ifdef __HIP_DEVICE_COMPILE__
    auto in_range = [](float a) {  // 2^-100 <= |a| <= 2^50 (on the magnitude's bits)
        return (uint32_t)((__float_as_uint(a) & 0x7fffffffu) - 0x0d800000u <= 0x58800000u - 0x0d800000u);
    };
    if (((uint32_t)(q >= 0x1p-80f) & (uint32_t)(q < 0x1p40f) & in_range(t.x) & in_range(t.y) & in_range(t.z))) {
        const RcpRef rr = rcp_ref(sqrt_unit(q));
        return F3{div_ref(t.x, rr), div_ref(t.y, rr), div_ref(t.z, rr)};
    }
#endif
    const float len = sqrtf(q);
    return F3{t.x / len, t.y / len, t.z / len};
}

// sample_sky, CPUPathTracer.cpp:286-292: glm::mix(horizon, zenith, t).
__device__ __forceinline__ F3 sample_sky(float dir_y, float4 horizon, float4 zenith) {
    const float t = 0.5f * (dir_y + 1.0f);
    const float s = 1.0f - t;
    return F3{horizon.x * s + zenith.x * t, horizon.y * s + zenith.y * t, horizon.z * s + zenith.z * t};
}

// Environment map on the miss path (superset; the reference's SkyBox,
// Scene.h:268-278, has no lookup): an octahedral map of w x h RGBA texels, nearest texel. The
// direction is projected onto the octahedron |x|+|y|+|z| = 1 (y up); the lower hemisphere is folded
// over the diagonals. Only +, -, *, / and fabs: the oracle restates it bit for bit.
__host__ __device__ inline uint32_t octa_texel(float dx, float dy, float dz, uint32_t w, uint32_t h) {
    const float s = (fabsf(dx) + fabsf(dy)) + fabsf(dz);
    float px = dx / s, pz = dz / s;
    if (dy < 0.0f) {
        const float fx = (1.0f - fabsf(pz)) * (px >= 0.0f ? 1.0f : -1.0f);
        const float fz = (1.0f - fabsf(px)) * (pz >= 0.0f ? 1.0f : -1.0f);
        px = fx;
        pz = fz;
    }
    // fmaxf/fminf drop a NaN (zero direction): it maps to texel 0
    const float u = fminf(fmaxf(px * 0.5f + 0.5f, 0.0f), 1.0f);
    const float v = fminf(fmaxf(pz * 0.5f + 0.5f, 0.0f), 1.0f);
    uint32_t ix = (uint32_t)(u * (float)w), iy = (uint32_t)(v * (float)h);
    ix = ix < w ? ix : w - 1u;
    iy = iy < h ? iy : h - 1u;
    return iy * w + ix;
}

// get_random_bounche, CPUPathTracer.cpp:303-326 (cosine-weighted hemisphere around n), split in
// two: the tangent t of the frame (a function of n only, so it can be computed once per primary
// hit and reused for every frame of a pixel) and the random direction around (n, t, n x t).
// (float)sqrt((double)u) == sqrtf(u) exactly for float u (double has > 2*24+2 bits), so the two
// square roots stay fp32; cos/sin and the products with sinTheta are fp64 as in the reference.
__host__ __device__ __forceinline__ F3 bounce_tangent(F3 n, uint32_t flags) {
    // `abs(normal.z) < 0.999f`: ::abs(int) under libstdc++ (truncate, then |i| < 0.999 <=> i == 0)
    const bool not_pole = (flags & kFlagAbsFloat) ? (fabsf(n.z) < 0.999f) : ((int)n.z == 0);
    const F3 up = not_pole ? F3{0.0f, 0.0f, 1.0f} : F3{1.0f, 0.0f, 0.0f};
    return normalize3(cross3(up, n));
}
// bounce_tangent without the window test of its inverse root (inv_sqrt_ranged), for the shading normal n of a
// hit in k_paths' step loop under spt_kernels.h flat_tangent_baked. x = |up x n|^2 is in [2^-96, 2^96):
//   - n = ng * inv_len with ng's squared length in the window (the call site's argument), so each component
//     carries at most 3 roundings and |n|^2 = 1 +- 2^-21; no component exceeds 1 + 2^-22, so x < 4.
//   - SPT_FLAG_ABS_FLOAT: off the pole (|n.z| < 0.999f) up = z and up x n = (-n.y, n.x, 0), so
//     x = n.x^2 + n.y^2 >= (1 - 2^-21) - 0.999^2 - 2^-21 > 2^-10; at the pole up = x and up x n = (0, -n.z, n.y),
//     so x >= n.z^2 (1 - 2^-23) > 0.99.
//   - without the flag the pole test is (int)n.z == 0, which a unit normal with n.z = 1 - 2^-24 and
//     n.x = n.y = 0 passes with x = 0: no bound holds for a normal computed on the device (a sphere's). The
//     form is then used only for a shape without spheres, whose normals are the stored ones: flat_ranges_ok
//     (scene.cpp) has evaluated this very x for each of them, in both forms, and found it inside.
__device__ __forceinline__ F3 bounce_tangent_ranged(F3 n, uint32_t flags) {
    const bool not_pole = (flags & kFlagAbsFloat) ? (fabsf(n.z) < 0.999f) : ((int)n.z == 0);
    const F3 up = not_pole ? F3{0.0f, 0.0f, 1.0f} : F3{1.0f, 0.0f, 0.0f};
    const F3 c = cross3(up, n);
    const float inv = inv_sqrt_ranged(dot3(c, c));
    return F3{c.x * inv, c.y * inv, c.z * inv};
}

// sin and cos of phi in [0, 2*pi] in fp64 (the reference calls the C double cos/sin here, see
// bounce_dir_frame). Cody-Waite reduction by pi/2 (k <= 4: k * kPio2Hi and phi - k * kPio2Hi are
// exact) and Taylor polynomials to r^15 / r^16 on |r| <= pi/4: truncation < 2^-53, so the result
// is within an ulp or so of the correctly rounded value, like the library routines. What the
// integrator consumes is (float)((double)sinTheta * cos), which agreed with glibc's cos/sin for
// all of 1e8 sampled (u1, u2) pairs. About a third of the fp64 work of the
// general-argument sincos (no large-argument path).
// The coefficients of sincos_2pi's polynomials (sin: [0..6], cos: [7..14]), highest power first.
#define SPT_SINCOS_COEFS                                                                              \
    -1.0 / 1307674368000.0, 1.0 / 6227020800.0, -1.0 / 39916800.0, 1.0 / 362880.0, -1.0 / 5040.0,     \
        1.0 / 120.0, -1.0 / 6.0, 1.0 / 20922789888000.0, -1.0 / 87178291200.0, 1.0 / 479001600.0,     \
        -1.0 / 3628800.0, 1.0 / 40320.0, -1.0 / 720.0, 1.0 / 24.0, -0.5
#ifdef __HIP_DEVICE_COMPILE__
// kSmemCoef: a kernel can only take a double constant as an operand from a register (gfx950 VOP3
// has no literals), so inline each of the 15 coefficients costs a v_mov_b64 per call. Read from this
// table through a pointer the compiler cannot hoist, they arrive by scalar loads (SMEM, no VALU) in
// SGPRs, which the FMAs take as operands directly, and free VGPRs: the BVH k_paths spills less
// (C4 +6 %). The flat k_paths uses the table too since round 3 (its step loop had come to spill the
// hoisted coefficient pairs: +3.9 % on C2). Same values, same FMAs: same bits.
static __constant__ double kSinCosCoef[16] = {SPT_SINCOS_COEFS, 0.0};
#endif
// fma(a, b, c) with c in an SGPR pair, as ONE VOP3 v_fma_f64. Left to itself the compiler picks the
// two-address v_fmac_f64 (dst += a * b) for every Horner step of sincos_2pi, and then has to copy the
// scalar-loaded coefficient into the destination VGPR pair first: two v_mov_b32 per step, 26 per
// sample. The same fused operation, so the same bits.
__device__ __forceinline__ double fma_sc(double a, double b, double c) {
#if defined(__HIP_DEVICE_COMPILE__)
    double r;
    asm("v_fma_f64 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "s"(c));
    return r;
#else
    return __builtin_fma(a, b, c);
#endif
}

// The unselected form: sr = sin(r), cr = cos(r) of the reduced argument and the quadrant q = k & 3, so that
// sin(phi), cos(phi) are (sr, cr), (cr, -sr), (-sr, -cr), (-cr, sr) for q = 0..3. sincos_2pi selects them as
// doubles; bounce_dir_xy's kLateQuadrant form selects after its products and conversions.
template <bool kSmemCoef = false>
__host__ __device__ inline void sincos_2pi_reduced(double phi, double& sr_out, double& cr_out, int& q_out) {
    constexpr double kPio2Hi = 1.57079632679489655800e+00;
    constexpr double kPio2Lo = 6.12323399573676603587e-17;
    constexpr double k2OverPi = 6.36619772367581382433e-01;
    constexpr double kInline[16] = {SPT_SINCOS_COEFS, 0.0};
#ifdef __HIP_DEVICE_COMPILE__
    const __attribute__((address_space(4))) double* cf = nullptr;
    if constexpr (kSmemCoef) {
        cf = (const __attribute__((address_space(4))) double*)kSinCosCoef;
        asm volatile("" : "+s"(cf));  // opaque: the loads stay next to their use (no SGPRs held across the loop)
    }
#define SPT_CF(i) (kSmemCoef ? cf[i] : kInline[i])
#else
#define SPT_CF(i) kInline[i]
#endif
    const double k = __builtin_rint(phi * k2OverPi);
    const double r = (phi - k * kPio2Hi) - k * kPio2Lo;
    const double w = r * r;
#if defined(__HIP_DEVICE_COMPILE__)
    // (the scalar-table coefficients as SGPR operands: fma_sc; the first step's C0 * w + C1 reads two
    // coefficients, and a VALU instruction takes one scalar operand, so it stays a plain fma)
#define SPT_HORNER(p, i) (kSmemCoef ? fma_sc(p, w, SPT_CF(i)) : __builtin_fma(p, w, SPT_CF(i)))
#else
#define SPT_HORNER(p, i) __builtin_fma(p, w, SPT_CF(i))
#endif
    double ps = SPT_CF(0);
    ps = __builtin_fma(ps, w, SPT_CF(1));
    ps = SPT_HORNER(ps, 2);
    ps = SPT_HORNER(ps, 3);
    ps = SPT_HORNER(ps, 4);
    ps = SPT_HORNER(ps, 5);
    ps = SPT_HORNER(ps, 6);
    const double sr = __builtin_fma(r * w, ps, r);
    double pc = SPT_CF(7);
    pc = __builtin_fma(pc, w, SPT_CF(8));
    pc = SPT_HORNER(pc, 9);
    pc = SPT_HORNER(pc, 10);
    pc = SPT_HORNER(pc, 11);
    pc = SPT_HORNER(pc, 12);
    pc = SPT_HORNER(pc, 13);
    pc = SPT_HORNER(pc, 14);
#undef SPT_HORNER
    const double cr = __builtin_fma(w, pc, 1.0);
    sr_out = sr;
    cr_out = cr;
    q_out = ((int)k) & 3;
#undef SPT_CF
}

template <bool kSmemCoef = false>
__host__ __device__ inline void sincos_2pi(double phi, double& s, double& c) {
    double sr, cr;
    int q;
    sincos_2pi_reduced<kSmemCoef>(phi, sr, cr, q);
    const double a = (q & 1) ? cr : sr;  // sin: sr, cr, -sr, -cr
    const double b = (q & 1) ? sr : cr;  // cos: cr, -sr, -cr, sr
    s = (q & 2) ? -a : a;
    c = ((q + 1) & 2) ? -b : b;
}

// Correctly rounded sqrtf for x = 0 and finite x >= 2^-96: hipcc's sqrtf sequence (hardware
// estimate, then the +-1 ulp residual corrections) without its rescaling of inputs below 2^-96 and
// its 0/inf pass-through, neither of which these inputs reach (sqrt(0): the estimate is 0 and both
// corrections keep it). Used for the random_float range [2^-32, 1] and by inv_sqrt_ref.
__host__ __device__ __forceinline__ float sqrt_unit(float x) {
#ifndef __HIP_DEVICE_COMPILE__
    return sqrtf(x);  // (the host build: the correctly rounded root itself)
#else
    const float s = __builtin_amdgcn_sqrtf(x);
    const float sm = __uint_as_float(__float_as_uint(s) - 1u);
    const float sp = __uint_as_float(__float_as_uint(s) + 1u);
    const float rm = __builtin_fmaf(-sm, s, x);
    const float rp = __builtin_fmaf(-sp, s, x);
    const float r = rm <= 0.0f ? sm : s;
    return rp > 0.0f ? sp : r;
#endif
}

// The tail of bounce_dir_frame: x = (float)((double)sin_t * cos(phi)), y = (float)((double)sin_t * sin(phi)).
// kLateQuadrant (k_paths' sampling site under the range bit): the quadrant's swap and signs are applied to the two
// converted floats instead of to the doubles sin and cos. The same bits for every finite sin_t and phi in [0, 2 pi]:
//   - The swap only chooses which of sr, cr a product takes, so it commutes with forming both products.
//   - A double product's and a conversion's rounding is round-to-nearest-even on the magnitude, the sign carried
//     apart: fl(s * (-a)) = -fl(s * a) and (float)(-v) = -(float)v for every finite s, a, v — zeros included
//     (s * (-a) is -0 exactly when s * a is +0), subnormal results included (the flush or not of a result does
//     not look at its sign). So (float)(sin_t * (-a)) and -(float)(sin_t * a) are the same word.
//   - No NaN arises (sin_t in [0, 1], |sr|, |cr| <= 1: the products are finite), so no payload or sign of a NaN
//     is in question.
// tests/cpp/test_quadrant_select.cpp compares the two forms on the host build for every quadrant and the floats
// around each multiple of pi / 2; the 32-bit select costs half the instructions of the 64-bit one.
template <bool kSmemCoef = false, bool kLateQuadrant = false>
__host__ __device__ __forceinline__ void bounce_dir_xy(float sin_t, float phi, float& x, float& y) {
#ifdef SPT_EXPERIMENT_FP32_TRIG  // measurement-only build: prices the fp64 trig; NOT reference numerics
    float spf, cpf;
    sincosf(phi, &spf, &cpf);
    x = sin_t * cpf;
    y = sin_t * spf;
#else
    if constexpr (kLateQuadrant) {
        double sr, cr;
        int q;
        sincos_2pi_reduced<kSmemCoef>((double)phi, sr, cr, q);
        const float fs = (float)((double)sin_t * sr);
        const float fc = (float)((double)sin_t * cr);
        const float a = (q & 1) ? fc : fs;  // sin: sr, cr, -sr, -cr
        const float b = (q & 1) ? fs : fc;  // cos: cr, -sr, -cr, sr
        y = (q & 2) ? -a : a;
        x = ((q + 1) & 2) ? -b : b;
    } else {
        double sp, cp;
        sincos_2pi<kSmemCoef>((double)phi, sp, cp);
        x = (float)((double)sin_t * cp);
        y = (float)((double)sin_t * sp);
    }
#endif
}

template <bool kSmemCoef = false, bool kLateQuadrant = false>
__host__ __device__ __forceinline__ F3 bounce_dir_frame(F3 n, F3 t, uint32_t& state) {
    const float u1 = random_float(state);
    const float u2 = random_float(state);
    const float cos_t = sqrt_unit(u1);
    const float sin_t = sqrt_unit(1.0f - u1);
    const float phi = 2.0f * kPiF * u2;
    float x, y;
    bounce_dir_xy<kSmemCoef, kLateQuadrant>(sin_t, phi, x, y);
    const float z = cos_t;
    const F3 b = cross3(n, t);
    return F3{(x * t.x + y * b.x) + z * n.x, (x * t.y + y * b.y) + z * n.y, (x * t.z + y * b.z) + z * n.z};
}

template <bool kSmemCoef = false>
__host__ __device__ __forceinline__ F3 bounce_dir(F3 n, uint32_t& state, uint32_t flags) {
    return bounce_dir_frame<kSmemCoef>(n, bounce_tangent(n, flags), state);
}

// ---- primitive tests (replace rtcIntersect1, CPUPathTracer.cpp:214-227) ----------------------
// Each returns the closest root t >= tmin of the ray against the primitive, or +inf.

// Ray-sphere, sphere.md:170-188 (a = d.d, b = 2 L.d, c = L.L - r^2), near root first.
__device__ __forceinline__ float isect_sphere(float4 s, F3 o, F3 d, float tmin) {
    const float lx = o.x - s.x, ly = o.y - s.y, lz = o.z - s.z;
    const float a = (d.x * d.x + d.y * d.y) + d.z * d.z;
    const float b = 2.0f * ((lx * d.x + ly * d.y) + lz * d.z);
    const float c = ((lx * lx + ly * ly) + lz * lz) - s.w * s.w;
    const float disc = b * b - 4.0f * a * c;
    if (!(disc >= 0.0f)) return kInf;
    const float sq = sqrtf(disc);
    const float two_a = 2.0f * a;
    const float t1 = (-b - sq) / two_a;
    if (t1 >= tmin) return t1;
    const float t2 = (-b + sq) / two_a;
    if (t2 >= tmin) return t2;
    return kInf;
}

// Russian roulette's ray_throughput /= p (CPUPathTracer.cpp:268), p = max(T) > 0: the three correctly
// rounded divisions by p as ONE refined reciprocal and three div_ref when every operand is in div_ref's
// range — p in [2^-40, 2^20], each T component 0 or in [2^-100, 2^50] (components are >= 0; 0 / p gives
// +0 either way) — else hipcc's division (a lane with a tiny component). Same bits; 3 v_div_scale pairs,
// fmas and fixups fewer.
__device__ __forceinline__ F3 rr_divide(F3 T, float p) {
    // the range predicates combined without short-circuits (`|`, `&`): one branch instead of a cascade
    // of five exec-mask branches (SALU)
    auto in_range = [](float c) { return (c == 0.0f) | (c >= 0x1p-100f); };
    const bool p_ok = (p >= 0x1p-40f) & (p <= 0x1p20f);
    if ((p_ok & in_range(T.x) & in_range(T.y) & in_range(T.z))) {
        const RcpRef r = rcp_ref(p);
        return F3{div_ref(T.x, r), div_ref(T.y, r), div_ref(T.z, r)};
    }
    return F3{T.x / p, T.y / p, T.z / p};
}

// rr_divide without its range predicates (8 compares and their mask arithmetic), for k_paths' step loop under
// spt_kernels.h flat_ranges_baked: a scene that passed flat_ranges_ok (scene.cpp) traced with max_bounces <= 9.
// Every operand is then in div_ref's range:
//   - T starts as 1 * albedo and is multiplied by one albedo per hit; roulette runs at bounce_count <
//     max_bounces, so T is a product of at most 8 albedos, with divisions by earlier p in between.
//   - An albedo component is 0 or in [2^-5, 1]. Rounding is monotone and powers of two are floats, so a product
//     of two components in [2^-a, 1] and [2^-b, 1] rounds into [2^-(a+b), 1]; a division by p in (0, 1] of a
//     component <= p rounds into [component, 1]. By induction each T component is 0 or in [2^-40, 1].
//   - Some channel is nonzero in every material, so that component of T is never 0 and p = max(T) is in
//     [2^-40, 1] (never the p == 0 whose 0 / 0 only the general division reproduces).
// So p is in [2^-40, 2^20] and each numerator is 0 or in [2^-100, 2^50]: rr_divide takes its first branch for
// every lane, and this is that branch. tests/cpp/test_device_ranges.hip compares it with '/' and rr_divide.
__device__ __forceinline__ F3 rr_divide_ranged(F3 T, float p) {
    const RcpRef r = rcp_ref(p);
    return F3{div_ref(T.x, r), div_ref(T.y, r), div_ref(T.z, r)};
}

// isect_sphere for |d| ~ 1 (a = d . d in [0.5, 2], two_a's reciprocal refined once per ray in
// r2a) in a scene that passed fast_division_ok (|center| + radius below 2^28): |-b -+ sq| < 2^31,
// so div_ref gives the same t (or both are below kTNear). sqrt_unit is exact for disc = 0 and disc >= 2^-96; a discriminant in (0, 2^-96)
// sets `redo` (the caller repeats the ray with isect_sphere).
// rr: s.w * s.w, precomputed by the host (scene.cpp prepare_prims, DevPrim b.x): the same product.
__device__ __forceinline__ float isect_sphere_fast(float4 s, float rr, F3 o, F3 d, float a, RcpRef r2a, float tmin,
                                                   bool& redo) {
    const float lx = o.x - s.x, ly = o.y - s.y, lz = o.z - s.z;
    const float b = 2.0f * ((lx * d.x + ly * d.y) + lz * d.z);
    const float c = ((lx * lx + ly * ly) + lz * lz) - rr;
    const float disc = b * b - 4.0f * a * c;
    // (the same predicates as `if (!(disc >= 2^-96)) { redo |= disc > 0; if (disc != 0) miss }`, without
    // the nested branch: lane masks, no exec-mask region)
    redo = redo | ((disc > 0.0f) & (disc < 0x1p-96f));
    if (!((disc >= 0x1p-96f) | (disc == 0.0f))) return kInf;
    const float sq = sqrt_unit(disc);
    const float t1 = div_ref(-b - sq, r2a);
    if (t1 >= tmin) return t1;
    const float t2 = div_ref(-b + sq, r2a);
    if (t2 >= tmin) return t2;
    return kInf;
}

// The minimum of two closest-hit keys, (t bits << 32) | original index, as unsigned integers: on the device ONE
// v_min_f64 on the keys read as doubles (the integer form compiles to a 64-bit compare, a wait state for its mask
// and two selects). kKeyMin = false: the integer form on the device too (spt_kernels.hip k_paths says for which
// kernels). Measured on C2 (profiles/key_min_rates.txt).
// Why the bits are the integer minimum's:
//   - Domain. A key's high word is __float_as_uint(t) with t >= the test's tmin > 0 or t = +inf (every test ends in
//     `cond ? t : kInf`, so a NaN t never reaches a key), or the caller's incoming best_t: kInf, or a shadow ray's
//     smax > 0. So the high word is in [1, 0x7f800000]: read as doubles, both operands are positive.
//   - Upper end. The high word is <= 0x7f800000 < 0x7ff00000: neither operand is a double NaN or infinity. Positive
//     finite doubles order as their bit patterns do, the IEEE mode's quieting of a signalling NaN cannot occur, and
//     v_min_f64 returns one operand's 64 bits unchanged.
//   - Lower end. A high word below 0x00100000 (a tiny smax) is a denormal double. The kernels run with fp64
//     denormals on (the AMDGPU default: .amdhsa_float_denorm_mode_16_64 3 in every kernel's descriptor), so a
//     denormal operand is compared and returned as it is, not flushed. tests/cpp/test_key_min.hip covers such words.
//   - Ties. Equal high words order by the low word, the original index; equal keys give the same bits either way.
// (Not __builtin_fmin: the compiler puts a canonicalizing v_max_f64 in front of each operand.)
template <bool kKeyMin = true>
__host__ __device__ __forceinline__ uint64_t key_min(uint64_t a, uint64_t b) {
#ifdef __HIP_DEVICE_COMPILE__
    if constexpr (kKeyMin) {
        double r;
        asm("v_min_f64 %0, %1, %2" : "=v"(r) : "v"(__longlong_as_double((long long)a)), "v"(__longlong_as_double((long long)b)));
        return (uint64_t)__double_as_longlong(r);
    }
#endif
    return a < b ? a : b;
}

// kNS >= 2 spheres (kp: their records, two words of float4 read per sphere: a = (center, radius), b = (r^2, -, -,
// original index)) against one ray, with ONE root stage per ray where that is enough; `best` is the running
// (t bits, original index) key. The result is the minimum over isect_sphere_fast of every sphere, bit for bit.
// Stage 1, every sphere: isect_sphere_fast's b, c, disc, `redo` and validity, the same operations in the same
// order. A sphere is a candidate for a lane if its disc is valid and not (b > 0 && c > 0). Such a culled sphere
// returns kInf from isect_sphere_fast: t1's numerator -b - sq is negative, and disc = fl(fl(b b) - fl(4 a c)) <=
// fl(b b) (a > 0, c > 0), whose correctly rounded root is |b| (radix 2; no underflow: a valid disc is 0 or >=
// 2^-96), so sq <= b and t2's numerator -b + sq is <= 0; div_ref keeps the sign, and both roots fail t >= tmin.
// Stage 2, once per ray: the lane's first candidate (b, disc and index selected lane-wise) runs the root stage
// of isect_sphere_fast on the same operands: the same t. The far root runs only in a wave where some lane's
// near root fell below tmin (a ray that starts inside or on its sphere).
// Second pass: a wave with a lane of two or more candidates runs the root stage again, on each lane's second
// candidate; with three or more spheres, a wave with a lane of three or more candidates then runs
// isect_sphere_fast over every sphere (a sphere tested twice changes nothing: the key minimum is idempotent).
// `second`: the counting kernels' counts in LDS (second[1] counts the second passes, one per wave), or null.
// kKeyMin: key_min's form of the minimum.
// kRedoMask: *redo_w also gathers the wave's lanes that set `redo`, from stage 1's compares' own lane masks (scalar
// instructions only, as `cm` below). Stage 1 evaluates the predicate for every sphere and the per-sphere loop of the
// third pass only repeats it on the same operands, so with `redo` false on entry *redo_w is __ballot(redo) at the
// end, which the compiler serves with a v_cndmask 0, 1 and a compare, `redo` being a value merged across the
// passes' branches. false: redo_w is not read.
template <uint32_t kNS, bool kKeyMin = true, bool kRedoMask = false>
__device__ __forceinline__ void flat_sphere_pass(const float4* __restrict__ kp, F3 o, F3 d, float a, RcpRef r2a, float tmin,
                                                 bool& redo, uint64_t& best, uint32_t* second, uint64_t* redo_w = nullptr) {
    // One root stage on per-lane operands; `on`: the lane holds a candidate (another lane's operands are those of
    // some sphere that is none of its candidates, its roots are not read: no exec-mask region). A candidate's
    // near root is kept if t >= tmin, else the far root replaces it (the wave then runs the far root) and is kept
    // if t >= tmin: isect_sphere_fast's result. lanes: the wave's lanes that are `on` (a mask in scalar registers).
    auto roots = [&](float sb, float sdisc, uint32_t sidx, bool on, uint64_t lanes) {
        const float sq = sqrt_unit(sdisc);
        float t = div_ref(-sb - sq, r2a);
        const bool low = !(t >= tmin);
        if ((__builtin_amdgcn_ballot_w64(low) & lanes) != 0ull) {
            asm volatile("" ::: "memory");  // (kept a branch: the compiler would otherwise run the far root in every wave)
            t = low ? div_ref(-sb + sq, r2a) : t;
        }
        t = (on & (t >= tmin)) ? t : kInf;
        const uint64_t key = ((uint64_t)__float_as_uint(t) << 32) | sidx;
        best = key_min<kKeyMin>(key, best);
    };
    float bk[kNS], dk[kNS];
    uint32_t ik[kNS];
    bool cand[kNS];
    uint64_t any = 0ull, many = 0ull, more = 0ull;  // lane masks (scalar registers): a candidate, two or more, three or more
#pragma unroll
    for (uint32_t k = 0; k < kNS; ++k) {
        const float4 s = kp[4 * k + 0], pb = kp[4 * k + 1];
        const float lx = o.x - s.x, ly = o.y - s.y, lz = o.z - s.z;
        const float b = 2.0f * ((lx * d.x + ly * d.y) + lz * d.z);
        const float c = ((lx * lx + ly * ly) + lz * lz) - pb.x;
        const float disc = b * b - 4.0f * a * c;
        redo = redo | ((disc > 0.0f) & (disc < 0x1p-96f));
        if constexpr (kRedoMask) *redo_w |= __builtin_amdgcn_ballot_w64(disc > 0.0f) & __builtin_amdgcn_ballot_w64(disc < 0x1p-96f);
        cand[k] = ((disc >= 0x1p-96f) | (disc == 0.0f)) & (!(b > 0.0f) | !(c > 0.0f));
        bk[k] = b;
        dk[k] = disc;
        ik[k] = __float_as_uint(pb.w);
        // (the same predicate from the compares' own lane masks: scalar instructions only)
        const uint64_t cm = (__builtin_amdgcn_ballot_w64(disc >= 0x1p-96f) | __builtin_amdgcn_ballot_w64(disc == 0.0f)) &
                            (__builtin_amdgcn_ballot_w64(!(b > 0.0f)) | __builtin_amdgcn_ballot_w64(!(c > 0.0f)));
        more |= cm & many;
        many |= cm & any;
        any |= cm;
    }
    // the lane's first candidate: the last sphere's operands unless an earlier sphere is a candidate
    float sb = bk[kNS - 1u], sdisc = dk[kNS - 1u];
    uint32_t sidx = ik[kNS - 1u];
    bool seen = cand[kNS - 1u];
#pragma unroll
    for (uint32_t k = kNS - 1u; k-- > 0u;) {
        sb = cand[k] ? bk[k] : sb;
        sdisc = cand[k] ? dk[k] : sdisc;
        sidx = cand[k] ? ik[k] : sidx;
        seen = seen | cand[k];
    }
    roots(sb, sdisc, sidx, seen, any);
    if (many != 0ull) {
        // the lane's second candidate: the last sphere's operands unless an earlier sphere is the second one
        bool one = cand[0], two = false;  // the lane's candidates up to sphere k: one or more, two or more
        bool next[kNS];
        next[0] = false;
#pragma unroll
        for (uint32_t k = 1; k < kNS; ++k) {
            next[k] = cand[k] & one & !two;
            two = two | (cand[k] & one);
            one = one | cand[k];
        }
        float sb2 = bk[kNS - 1u], sdisc2 = dk[kNS - 1u];
        uint32_t sidx2 = ik[kNS - 1u];
#pragma unroll
        for (uint32_t k = kNS - 1u; k-- > 1u;) {
            sb2 = next[k] ? bk[k] : sb2;
            sdisc2 = next[k] ? dk[k] : sdisc2;
            sidx2 = next[k] ? ik[k] : sidx2;
        }
        roots(sb2, sdisc2, sidx2, two, many);
        // (one count per wave: the first active lane's, in LDS)
        if (second && __lane_id() == (uint32_t)__ffsll((long long)__ballot(true)) - 1u) atomicAdd(second + 1, 1u);
        if constexpr (kNS >= 3u) {
            if (more != 0ull) {
#pragma unroll
                for (uint32_t k = 0; k < kNS; ++k) {
                    const float4 s = kp[4 * k + 0], pb = kp[4 * k + 1];
                    const float tk = isect_sphere_fast(s, pb.x, o, d, a, r2a, tmin, redo);
                    const uint64_t kk = ((uint64_t)__float_as_uint(tk) << 32) | __float_as_uint(pb.w);
                    best = key_min<kKeyMin>(kk, best);
                }
            }
        }
    }
}

__device__ __forceinline__ float comp(float4 v, int i) { return i == 0 ? v.x : (i == 1 ? v.y : v.z); }
__device__ __forceinline__ float comp(F3 v, int i) { return i == 0 ? v.x : (i == 1 ? v.y : v.z); }

// Parallelogram whose normal lies along axis AX and whose edges lie in the plane (scene.cpp sets
// c.w = AX + 1): the plane is x[AX] = Q[AX], so t = (Q[AX] - o[AX]) / d[AX] (the build's definition
// of the axis-aligned quad; the oracle's isect_quad has the same form). The in-plane test is the
// general one with its exactly-zero terms dropped: each dropped term is a product with a +-0
// component of A or B, so every sum keeps its value except possibly the sign of a zero result,
// compared alike as x + 0.0f. d[AX] = +-0 gives t = +-inf or NaN, rejected as in the general form.
template <int AX>
__device__ __forceinline__ float isect_quad_axis(float4 pa, float4 pb, float4 pc, float4 pd, F3 o, F3 d, float tmin) {
    constexpr int U = AX == 0 ? 1 : 0;  // the two in-plane axes, in the general formula's order
    constexpr int V = AX == 2 ? 1 : 2;
    (void)pb;
    const float t = (comp(pa, AX) - comp(o, AX)) / comp(d, AX);
    if (!(t >= tmin) || t == kInf) return kInf;
    const float hu = (comp(o, U) + t * comp(d, U)) - comp(pa, U);
    const float hv = (comp(o, V) + t * comp(d, V)) - comp(pa, V);
    const float al = hu * comp(pc, U) + hv * comp(pc, V);
    const float be = hu * comp(pd, U) + hv * comp(pd, V);
    const uint32_t ua = __float_as_uint(al + 0.0f), ub = __float_as_uint(be + 0.0f);
    return max(ua, ub) <= 0x3f800000u ? t : kInf;
}

// isect_quad_axis with the unscaled division by d[AX] (its reciprocal refined once per ray in rAX),
// for |d[AX]| in [2^-20, 1.5] in a scene that passed fast_division_ok (coordinates below 2^28, so
// |o| < 2^28 + 1 and |Q[AX] - o[AX]| < 2^30): div_ref's quotient is the exact one (or both are below
// kTNear), and it is finite, so the t == inf test of the general form is dropped.
// The in-plane test runs for every lane (t is finite here): no exec-mask branch.
// kRect: the quad is known to be a rectangle (its group in a shape-specialized kernel, flat_rect_bits):
// the short form without the scalar check.
template <int AX, bool kRect = false>
__device__ __forceinline__ float isect_quad_axis_fast(float4 pa, float4 pc, float4 pd, F3 o, F3 d, RcpRef rAX,
                                                      float tmin) {
    constexpr int U = AX == 0 ? 1 : 0;
    constexpr int V = AX == 2 ? 1 : 2;
    const float t = div_ref(comp(pa, AX) - comp(o, AX), rAX);
    const float hu = (comp(o, U) + t * comp(d, U)) - comp(pa, U);
    const float hv = (comp(o, V) + t * comp(d, V)) - comp(pa, V);
    float al, be;
    // A rectangle whose edges also lie along the axes (a wall of a box: A = (a, 0), B = (0, b) in the
    // plane, every record word wave-uniform, so this is a scalar branch): the two products with a
    // zero component are dropped. hv * (+-0) is +-0 (hv is finite here), so the sum loses at most
    // the sign of a zero result, which x + 0.0f below erases: the same predicate.
    if (kRect || (((__float_as_uint(comp(pc, V)) | __float_as_uint(comp(pd, U))) & 0x7fffffffu) == 0u)) {
        al = hu * comp(pc, U);
        be = hv * comp(pd, V);
    } else {
        al = hu * comp(pc, U) + hv * comp(pc, V);
        be = hu * comp(pd, U) + hv * comp(pd, V);
    }
    const uint32_t ua = __float_as_uint(al + 0.0f), ub = __float_as_uint(be + 0.0f);
    return (t >= tmin && max(ua, ub) <= 0x3f800000u) ? t : kInf;
}

// isect_quad_axis_fast<AX, true> on the five record words it reads — q = a[AX], qu = a[U], qv = a[V],
// cu = c[U], dv = d[V] — with the same operations in the same order: the same bits. For a wall whose
// words are per-lane values (the paired test of closest_flat picks one wall of an opposite pair per lane).
template <int AX>
__device__ __forceinline__ float isect_rect_axis_fast(float q, float qu, float qv, float cu, float dv, F3 o, F3 d,
                                                      RcpRef rAX, float tmin) {
    constexpr int U = AX == 0 ? 1 : 0;
    constexpr int V = AX == 2 ? 1 : 2;
    const float t = div_ref(q - comp(o, AX), rAX);
    const float hu = (comp(o, U) + t * comp(d, U)) - qu;
    const float hv = (comp(o, V) + t * comp(d, V)) - qv;
    const float al = hu * cu;
    const float be = hv * dv;
    const uint32_t ua = __float_as_uint(al + 0.0f), ub = __float_as_uint(be + 0.0f);
    return (t >= tmin && max(ua, ub) <= 0x3f800000u) ? t : kInf;
}

// Parallelogram: a = (Q, D = n.Q), b = (n, -), c = (A, type | axis << 2), d = (B, -) (see scene.h).
__device__ __forceinline__ float isect_quad(float4 pa, float4 pb, float4 pc, float4 pd, F3 o, F3 d,
                                            float tmin) {
    const uint32_t axis = __float_as_uint(pc.w) >> 2;
    if (axis == 1u) return isect_quad_axis<0>(pa, pb, pc, pd, o, d, tmin);
    if (axis == 2u) return isect_quad_axis<1>(pa, pb, pc, pd, o, d, tmin);
    if (axis == 3u) return isect_quad_axis<2>(pa, pb, pc, pd, o, d, tmin);
    const float denom = (pb.x * d.x + pb.y * d.y) + pb.z * d.z;
    const float t = (pa.w - ((pb.x * o.x + pb.y * o.y) + pb.z * o.z)) / denom;
    if (!(t >= tmin) || t == kInf) return kInf;
    const float hx = (o.x + t * d.x) - pa.x;
    const float hy = (o.y + t * d.y) - pa.y;
    const float hz = (o.z + t * d.z) - pa.z;
    const float al = (hx * pc.x + hy * pc.y) + hz * pc.z;
    const float be = (hx * pd.x + hy * pd.y) + hz * pd.z;
    // (al >= 0 && al <= 1 && be >= 0 && be <= 1) on the bit patterns: for x + 0.0f (-0 -> +0),
    // 0 <= x <= 1 <=> bits(x) <= bits(1.0f); negatives, NaN and inf all compare above.
    const uint32_t ua = __float_as_uint(al + 0.0f), ub = __float_as_uint(be + 0.0f);
    return max(ua, ub) <= 0x3f800000u ? t : kInf;
}

// Moller-Trumbore: a = (v0, -), b = (e1, -), c = (e2, -).
__device__ __forceinline__ float isect_tri(float4 pa, float4 pb, float4 pc, F3 o, F3 d, float tmin) {
    const float px = d.y * pc.z - pc.y * d.z;
    const float py = d.z * pc.x - pc.z * d.x;
    const float pz = d.x * pc.y - pc.x * d.y;
    const float det = (pb.x * px + pb.y * py) + pb.z * pz;
    const float inv = recip_ref(det);  // (1.0f / det, the same bits)
    const float tx = o.x - pa.x, ty = o.y - pa.y, tz = o.z - pa.z;
    const float u = ((tx * px + ty * py) + tz * pz) * inv;
    if (!(u >= 0.0f && u <= 1.0f)) return kInf;
    const float qx = ty * pb.z - pb.y * tz;
    const float qy = tz * pb.x - pb.z * tx;
    const float qz = tx * pb.y - pb.x * ty;
    const float v = ((d.x * qx + d.y * qy) + d.z * qz) * inv;
    if (!(v >= 0.0f && u + v <= 1.0f)) return kInf;
    const float t = ((pc.x * qx + pc.y * qy) + pc.z * qz) * inv;
    if (!(t >= tmin) || t == kInf) return kInf;
    return t;
}


// ---- next-event estimation (SPT_FLAG_NEE; superset; oracle ref_light_sample) ----
// Emitter records (scene.cpp build_emitters), 5 float4 each:
//   (base.xyz, 1: triangle | 0: parallelogram), (e1.xyz, area * n_emitters / pi), (e2.xyz, 0),
//   (unit normal.xyz, 0), (emission.rgb, 0);
//   a sphere: (center.xyz, 2), (r, 0, 0, area * n_emitters / pi), 0, 0, (emission.rgb, 0)
constexpr uint32_t kEmitRecs = 5;
constexpr float kShadowFar = 0.999f;  // the shadow ray stops short of the sampled point: t < 0.999 * dist

// Three draws (emitter, u, v) at the offset hit point x with shading normal n and throughput T (after
// the albedo, before Russian roulette): the shadow ray direction w and its tmax, and the estimate
// T * (Le * g) with g = cos_s * cos_l * area * n_emit / (pi * dist^2). False when the point is behind
// either surface (no shadow ray). Correctly rounded sqrtf and '/', no contraction: the oracle's bits.
// kSpheres = false: a table without sphere records (the sphere sample left out of the kernel).
template <bool kSpheres = true>
__device__ __forceinline__ bool light_sample(const float4* __restrict__ emit, uint32_t n_emit, F3 x, F3 n, F3 T,
                                             uint32_t& rng, F3& w, float& tmax, F3& add) {
    const float u0 = random_float(rng);
    const float u1 = random_float(rng);
    const float u2 = random_float(rng);
    uint32_t j = (uint32_t)(u0 * (float)n_emit);
    j = j < n_emit ? j : n_emit - 1u;
    const float4* e = emit + kEmitRecs * j;
    const float4 e0 = e[0], e1 = e[1], e2 = e[2], e3 = e[3], e4 = e[4];
    const uint32_t kind = __float_as_uint(e0.w);
    F3 p, nl;
    if (kSpheres && kind == 2u) {
        // a sphere, uniform over its area: the unit normal (sz, s cos phi, s sin phi) from z = 1 - 2 u1,
        // s = sqrt(1 - z^2), phi = 2 pi u2 with bounce_dir's fp64 sincos (glibc's cos / sin, the
        // oracle's), the point center + r * normal
        const float z = 1.0f - 2.0f * u1;
        const float s = sqrt_unit(1.0f - z * z);  // (0, or in [2^-24, 1]: correctly rounded)
        const float phi = 2.0f * kPiF * u2;
        double sp, cp;
        sincos_2pi<true>((double)phi, sp, cp);
        nl = F3{(float)((double)s * cp), (float)((double)s * sp), z};
        p = F3{e0.x + e1.x * nl.x, e0.y + e1.x * nl.y, e0.z + e1.x * nl.z};
    } else {
        float a = u1, b = u2;
        if (kind != 0u) {  // uniform on the triangle
            const float su = sqrtf(u1);
            a = su * (1.0f - u2);
            b = su * u2;
        }
        p = F3{(e0.x + a * e1.x) + b * e2.x, (e0.y + a * e1.y) + b * e2.y, (e0.z + a * e1.z) + b * e2.z};
        nl = F3{e3.x, e3.y, e3.z};
    }
    const F3 v{p.x - x.x, p.y - x.y, p.z - x.z};
    const float d2 = dot3(v, v);
    const float dist = sqrtf(d2);
    const float inv = 1.0f / dist;
    w = F3{v.x * inv, v.y * inv, v.z * inv};
    const float cs = dot3(n, w);
    // a sphere emits towards x from the side x sees: its outside when x is outside (the far side is
    // occluded by the sphere itself), its inside when x is inside (a dome around the scene);
    // parallelograms and triangles from both
    const float dl = dot3(nl, w);
    float cl = fabsf(dl);
    if (kSpheres && kind == 2u) {
        const F3 xc{x.x - e0.x, x.y - e0.y, x.z - e0.z};
        cl = dot3(xc, xc) < e1.x * e1.x ? dl : -dl;
    }
    if (!(cs > 0.0f) || !(cl > 0.0f)) return false;
    const float g = ((cs * cl) * e1.w) / d2;
    tmax = dist * kShadowFar;
    add = F3{T.x * (e4.x * g), T.y * (e4.y * g), T.z * (e4.z * g)};
    return true;
}

// ---- materials (spt_set_material_models; superset: the reference shades one Lambertian 0.7) ----------
// A material's model travels in one word that was zero before, DevMaterial::albedo[3] (scene.h; the flat
// scenes' LDS shading record carries it as alb.w): +0.0f is DIFFUSE, a float with the sign bit set is
// METAL with fuzz = |word| (-0.0f: a mirror), any other value is DIELECTRIC with that index of refraction
// (finite and > 0). Lossless: the kernels compute with the caller's parameter bits.
constexpr uint32_t kMatDiffuse = 0u, kMatMetal = 1u, kMatDielectric = 2u;  // spt_material_kind
__host__ __device__ __forceinline__ uint32_t model_kind(uint32_t word) {
    return word == 0u ? kMatDiffuse : ((word >> 31) ? kMatMetal : kMatDielectric);
}

// The scattering step of a METAL or DIELECTRIC hit (spt.h "materials" states the expressions): d the
// incoming direction, nf the unit normal on the side the ray arrives from, `entering` whether the ray
// goes from outside in. fp32, no contraction, correctly rounded sqrtf and '/', normalize3's 1 / sqrt.
// METAL(f): r = d - (2 (d . nf)) nf, plus f times a cosine-weighted direction around nf when f > 0 (two
// draws), normalized; absorbed unless r . nf > 0. DIELECTRIC(ior): one draw u; Snell with Schlick's
// reflectance; total internal reflection or R > u reflects as METAL(0), else the refracted direction,
// normalized (`transmitted`: the next origin lies on the far side). The host (spt_bsdf_sample) and every
// kernel compile this one function.
struct Scatter {
    F3 dir;
    bool transmitted, absorbed;
};
template <bool kSmemCoef = false>
__host__ __device__ inline Scatter bsdf_scatter(uint32_t kind, float param, F3 d, F3 nf, bool entering, uint32_t flags,
                                                uint32_t& rng) {
    float fuzz = 0.0f;
    if (kind == kMatDielectric) {
        const float ior = param;
        const float u = random_float(rng);
        const float eta = entering ? 1.0f / ior : ior;
        const float ci = fminf(-dot3(d, nf), 1.0f);
        const float s2 = fmaxf(1.0f - ci * ci, 0.0f);
        const float k = (eta * eta) * s2;
        const float ct = sqrtf(fmaxf(1.0f - k, 0.0f));
        const float q = (1.0f - ior) / (1.0f + ior);
        const float r0 = q * q;
        const float x = 1.0f - (entering ? ci : ct);
        const float x2 = x * x;
        const float R = r0 + (1.0f - r0) * ((x2 * x2) * x);
        if (!(k > 1.0f || R > u)) {
            const F3 t{eta * (d.x + ci * nf.x) - ct * nf.x, eta * (d.y + ci * nf.y) - ct * nf.y,
                       eta * (d.z + ci * nf.z) - ct * nf.z};
            return Scatter{normalize3(t), true, false};
        }
    } else {
        fuzz = param;
    }
    const float c2 = 2.0f * dot3(d, nf);
    F3 r{d.x - c2 * nf.x, d.y - c2 * nf.y, d.z - c2 * nf.z};
    if (fuzz > 0.0f) {
        const F3 b = bounce_dir<kSmemCoef>(nf, rng, flags);
        r = F3{r.x + fuzz * b.x, r.y + fuzz * b.y, r.z + fuzz * b.z};
    }
    r = normalize3(r);
    return Scatter{r, false, !(dot3(r, nf) > 0.0f)};
}

__device__ __forceinline__ uint32_t meta_type(float4 pd) { return __float_as_uint(pd.w) & 3u; }
__device__ __forceinline__ uint32_t meta_material(float4 pd) { return __float_as_uint(pd.w) >> 2; }

}  // namespace spt
