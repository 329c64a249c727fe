// GPU check of spt_device.h's guard-free forms (the k_paths step loop of a scene that passed scene.cpp
// flat_ranges_ok) against '/', sqrtf and the guarded forms, over exactly the ranges their comments prove:
//   inv_sqrt_ranged(x) == 1.0f / sqrtf(x) == inv_sqrt_ref(x) for EVERY float in [2^-96, 2^96);
//   rr_divide_ranged(T, p) == T / p == rr_divide(T, p) for EVERY p in [2^-40, 1] against components that are 0,
//     p itself, 2^-40, the floats next to those, and hashed values in [2^-40, p];
//   0.0f + 1.0f * e == e bit for bit for EVERY e >= +0 (+inf included), the path start's emission;
//   bounce_tangent_ranged(n) == bounce_tangent(n) on 2^26 hashed unit normals and on normals at both pole
//     tests' thresholds: with SPT_FLAG_ABS_FLOAT every one, without it those whose |up x n|^2 lies in
//     [2^-90, 2^90] (what flat_ranges_ok admits for a stored normal; the others are counted, not compared);
//   a sphere of the smallest admitted radius, r = E / 32, hit centrally from anywhere in the scene's box: the
//     computed |hit - centre|^2 stays >= r^2 / 17 and inside the window (the bound the shading normal leans on).
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>

#include "spt_device.h"

__device__ __forceinline__ bool same_bits(float a, float b) { return __float_as_uint(a) == __float_as_uint(b); }

__device__ __forceinline__ uint32_t hash32(uint32_t x) {
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}

// input i: the float with bits lo + i, for i < n
__global__ void k_check_inv_sqrt(uint32_t lo, uint32_t base, uint32_t n, unsigned long long* bad) {
    const uint32_t i = base + blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float x = __uint_as_float(lo + i);
    const float a = spt::inv_sqrt_ranged(x);
    if (!same_bits(a, 1.0f / sqrtf(x)) || !same_bits(a, spt::inv_sqrt_ref(x))) atomicAdd(bad, 1ull);
}

// divisor i of the enumeration: bits(2^-40) + i, up to 1.0f
__global__ void k_check_rr(uint32_t lo, uint32_t base, uint32_t n, unsigned long long* bad) {
    const uint32_t i = base + blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float p = __uint_as_float(lo + i);
    // components in {0} u [2^-40, p]: the edges, their neighbours inside the range, and hashed values
    float c[9];
    c[0] = 0.0f;
    c[1] = p;
    c[2] = 0x1p-40f;
    c[3] = __uint_as_float(max(lo, lo + i - 1u));  // the float below p (p itself at the range's lower end)
    c[4] = __uint_as_float(min(lo + 1u, lo + i));  // the float above 2^-40 (p itself where that exceeds p)
    for (uint32_t k = 5; k < 9u; ++k) c[k] = __uint_as_float(lo + hash32(i * 4u + k + 0x51ed27u) % (i + 1u));
    for (uint32_t k = 0; k < 9u; k += 3u) {
        const spt::F3 T{c[k], c[(k + 4u) % 9u], c[(k + 8u) % 9u]};
        const spt::F3 q = spt::rr_divide_ranged(T, p), g = spt::rr_divide(T, p);
        if (!same_bits(q.x, T.x / p) || !same_bits(q.y, T.y / p) || !same_bits(q.z, T.z / p) || !same_bits(q.x, g.x) ||
            !same_bits(q.y, g.y) || !same_bits(q.z, g.z))
            atomicAdd(bad, 1ull);
    }
}

// every e >= +0: bits 0 .. bits(+inf)
__global__ void k_check_emission(uint32_t base, uint32_t n, unsigned long long* bad) {
    const uint32_t i = base + blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float e = __uint_as_float(i);
    volatile float zero = 0.0f, one = 1.0f;  // (the sum as the kernels form it, not folded here)
    if (!same_bits(zero + one * e, e)) atomicAdd(bad, 1ull);
}

__device__ __forceinline__ bool tangent_in_window(spt::F3 n, uint32_t flags) {
    const bool not_pole = (flags & spt::kFlagAbsFloat) ? (fabsf(n.z) < 0.999f) : ((int)n.z == 0);
    const spt::F3 up = not_pole ? spt::F3{0.0f, 0.0f, 1.0f} : spt::F3{1.0f, 0.0f, 0.0f};
    const spt::F3 c = spt::cross3(up, n);
    const float x = spt::dot3(c, c);
    return x >= 0x1p-90f && x <= 0x1p90f;
}

// input i: a unit normal n = ng * inv_sqrt_ref(|ng|^2), as shade_hit forms it. The first 4096 inputs sit at
// the pole tests: n.z around +-0.999f and +-1 with small or zero n.x, n.y; the rest are hashed directions.
// out[0]: mismatches, out[1]: normals the form without the flag does not admit (not compared),
// out[2]: SPT_FLAG_ABS_FLOAT normals outside the window (the proof says none)
__global__ void k_check_tangent(uint32_t n_in, unsigned long long* out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_in) return;
    const uint32_t h0 = hash32(3u * i), h1 = hash32(3u * i + 1u), h2 = hash32(3u * i + 2u);
    spt::F3 ng;
    if (i < 4096u) {
        const float z = (i & 1u) ? 0.999f : 1.0f;
        const float zz = __uint_as_float(__float_as_uint(z) + ((i >> 1) & 7u) - 4u) * ((i & 16u) ? -1.0f : 1.0f);
        const float s = (i & 32u) ? 0.0f : __uint_as_float(((127u - (h0 % 60u)) << 23) | (h1 & 0x7fffffu));
        ng = spt::F3{(i & 64u) ? s : 0.0f, (i & 128u) ? s : -s, zz};
        if (i & 256u) {  // scaled, so that the normalization rounds
            const float k = 1.0f + (float)(h2 & 1023u) / 64.0f;
            ng = spt::F3{ng.x * k, ng.y * k, ng.z * k};
        }
    } else {
        auto comp = [](uint32_t h) { return ((float)(h >> 8) / 8388608.0f - 1.0f) * (float)(1u + (h & 7u)); };
        ng = spt::F3{comp(h0), comp(h1), comp(h2)};
    }
    const float nn = ng.x * ng.x + ng.y * ng.y + ng.z * ng.z;
    if (!(nn >= 0x1p-90f && nn <= 0x1p90f)) return;
    const float inv = spt::inv_sqrt_ref(nn);
    const spt::F3 n{ng.x * inv, ng.y * inv, ng.z * inv};
    for (uint32_t flags = 0; flags < 2u; ++flags) {
        if (!tangent_in_window(n, flags)) {
            atomicAdd(out + (flags ? 2 : 1), 1ull);
            continue;
        }
        const spt::F3 a = spt::bounce_tangent_ranged(n, flags), b = spt::bounce_tangent(n, flags);
        if (!same_bits(a.x, b.x) || !same_bits(a.y, b.y) || !same_bits(a.z, b.z)) atomicAdd(out, 1ull);
    }
}

// The shading normal of a sphere at the smallest radius flat_ranges_ok admits, r = E / 32 (E: the scene's
// coordinate bound): ray i starts at a hashed point of the box [-E, E]^3 and aims at a hashed point within
// r * 2^-k of the sphere's centre (k = i mod 24: central hits to within rounding, the case the bound is about),
// its direction normalized as the integrator's are. Both intersectors run (isect_sphere_fast with its `redo`
// protocol, and the general isect_sphere); for each hit the shade_hit expressions form the hit point and
// Ng = hit - centre, and |Ng|^2 must be >= r^2 / 17 (the comment at shade_hit proves |Ng| >= r / 4) and inside
// inv_sqrt_ranged's window. out[0]: hits checked, out[1]: violations; min_ratio: the smallest |Ng|^2 / r^2 seen.
__global__ void k_check_sphere_normal(float E, uint32_t n_in, unsigned long long* out, unsigned int* min_ratio) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_in) return;
    auto unit = [](uint32_t h) { return (float)(h >> 8) / 8388608.0f - 1.0f; };  // [-1, 1)
    const float r = E / 32.0f, rr = r * r;
    // the centre: anywhere with |c| + r <= E per coordinate
    const float cs = E - r;
    const float4 s = make_float4(unit(hash32(7u * i)) * cs, unit(hash32(7u * i + 1u)) * cs, unit(hash32(7u * i + 2u)) * cs, r);
    const spt::F3 o{unit(hash32(7u * i + 3u)) * E, unit(hash32(7u * i + 4u)) * E, unit(hash32(7u * i + 5u)) * E};
    const uint32_t h6 = hash32(7u * i + 6u);
    const float off = r * __uint_as_float((127u - (i % 24u)) << 23);
    const spt::F3 aim{s.x + unit(hash32(h6)) * off, s.y + unit(hash32(h6 + 1u)) * off, s.z + unit(hash32(h6 + 2u)) * off};
    const spt::F3 v{aim.x - o.x, aim.y - o.y, aim.z - o.z};
    const float vv = spt::dot3(v, v);
    if (!(vv >= 0x1p-90f)) return;
    const spt::F3 d = spt::normalize3(v);
    const float a = (d.x * d.x + d.y * d.y) + d.z * d.z;
    bool redo = false;
    const float tf = spt::isect_sphere_fast(s, rr, o, d, a, spt::rcp_ref(2.0f * a), spt::kTNear, redo);
    const float tg = spt::isect_sphere(s, o, d, spt::kTNear);
    const float ts[2] = {redo ? tg : tf, tg};
    for (int k = 0; k < 2; ++k) {
        const float t = ts[k];
        if (!(t < spt::kInf)) continue;
        const spt::F3 hit{o.x + t * d.x, o.y + t * d.y, o.z + t * d.z};
        const spt::F3 ng{hit.x - s.x, hit.y - s.y, hit.z - s.z};
        const float x = ng.x * ng.x + ng.y * ng.y + ng.z * ng.z;
        atomicAdd(out, 1ull);
        if (!(x >= rr / 17.0f) || !(x >= 0x1p-96f && x < 0x1p96f)) atomicAdd(out + 1, 1ull);
        atomicMin(min_ratio, __float_as_uint(x / rr));
    }
}

static uint32_t bits_of(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}

int main() {
    unsigned long long* d = nullptr;
    if (hipMalloc(&d, 12 * sizeof(*d)) != hipSuccess || hipMemset(d, 0, 12 * sizeof(*d)) != hipSuccess) return 2;
    const unsigned int inf_bits = 0x7f800000u;
    if (hipMemcpy(d + 8, &inf_bits, sizeof(inf_bits), hipMemcpyHostToDevice) != hipSuccess) return 2;
    const uint32_t per = 1u << 26;
    {
        const uint32_t lo = bits_of(0x1p-96f), n = bits_of(0x1p96f) - lo;  // [2^-96, 2^96)
        for (uint64_t b = 0; b < n; b += per) k_check_inv_sqrt<<<per / 256u, 256>>>(lo, (uint32_t)b, n, d + 0);
        std::printf("inv_sqrt_ranged: %u inputs in [2^-96, 2^96)\n", n);
    }
    {
        const uint32_t lo = bits_of(0x1p-40f), n = bits_of(1.0f) - lo + 1u;  // [2^-40, 1]
        for (uint64_t b = 0; b < n; b += per) k_check_rr<<<per / 256u, 256>>>(lo, (uint32_t)b, n, d + 1);
        std::printf("rr_divide_ranged: %u divisors in [2^-40, 1] x 3 throughputs\n", n);
    }
    {
        const uint32_t n = 0x7f800000u + 1u;  // +0 .. +inf
        for (uint64_t b = 0; b < n; b += per) k_check_emission<<<per / 256u, 256>>>((uint32_t)b, n, d + 2);
        std::printf("emission: %u values >= +0\n", n);
    }
    k_check_tangent<<<per / 256u, 256>>>(per, d + 3);
    {
        const float extents[] = {1.0f, 8.0f, 1000.0f, 0x1p27f};  // scenes of four scales, up to fast_division_ok's bound
        for (float E : extents) k_check_sphere_normal<<<(1u << 22) / 256u, 256>>>(E, 1u << 22, d + 6, (unsigned int*)(d + 8));
    }
    unsigned long long h[12];
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(h, d, sizeof(h), hipMemcpyDeviceToHost) != hipSuccess) return 2;
    std::printf("mismatches: inv_sqrt %llu, rr_divide %llu, emission %llu, tangent %llu\n", h[0], h[1], h[2], h[3]);
    std::printf("tangent: %llu normals outside the window without SPT_FLAG_ABS_FLOAT (skipped), %llu with it\n", h[4], h[5]);
    float min_ratio;
    const unsigned int mr = (unsigned int)h[8];
    std::memcpy(&min_ratio, &mr, 4);
    std::printf("sphere normal at r = E / 32: %llu hits, %llu with |Ng|^2 below r^2 / 17 or outside the window; smallest |Ng|^2 / r^2 %.6f\n",
                h[6], h[7], min_ratio);
    (void)hipFree(d);
    const bool ok = h[0] == 0 && h[1] == 0 && h[2] == 0 && h[3] == 0 && h[5] == 0 && h[7] == 0 && h[6] > (1ull << 22);
    std::printf(ok ? "PASS\n" : "FAIL\n");
    return ok ? 0 : 1;
}
