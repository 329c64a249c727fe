// GPU check of the one-pass sphere test of the shape-specialized flat closest hit (spt_device.h flat_sphere_pass)
// against the per-sphere loop over isect_sphere_fast, for 2^24 (ray, three spheres) inputs:
//   - a sphere with b > 0 && c > 0 (the cull of stage 1) returns kInf from isect_sphere_fast, whatever its disc;
//   - flat_sphere_pass<3> over the three spheres, and flat_sphere_pass<2> over the first two, give the same
//     (t bits, original index) and the same `redo` as the loop, from the same starting key.
// The inputs are made from their index alone (make_input, the same function on the host and on the device), a
// wave of 64 at a time of one kind: random rays; rays starting 1e-4 off a sphere and leaving it at grazing
// angles, inside a second sphere; geometry of size 2^-49 (|b| near 2^-48, disc around 2^-96); crafted records with
// disc = 0 and disc within 4 ulps of 2^-96 on either side; geometry of size 2^27 (|b| up to 2^30); an exact
// duplicate and a concentric sphere around the origin of the ray; three spheres in a row along the ray. In every
// other group of eight waves all spheres but one lie behind the ray (b > 0, c > 0), so no lane has two candidates
// and the wave's answer comes from the one root stage alone; the count of second passes shows both kinds ran.
// `--host` launches nothing: it builds the same inputs, evaluates stage 1 in host arithmetic (the same +, -, *
// under -ffp-contract=off) and prints how many inputs reach each case the kernel is aimed at.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>

#include "spt_device.h"

using namespace spt;

namespace {

constexpr uint32_t kInputs = 1u << 24;
constexpr uint32_t kKinds = 8;
constexpr uint32_t kNS = 3;

struct Input {
    F3 o, d;
    float4 rec[4 * kNS];  // per sphere the record's first two words: (center, radius), (r^2, -, -, index bits)
};

__host__ __device__ inline uint32_t hash32(uint32_t x) {  // (the PCG output function over an LCG step)
    x = x * 747796405u + 2891336453u;
    x = ((x >> ((x >> 28) + 4u)) ^ x) * 277803737u;
    return (x >> 22) ^ x;
}
struct Rng {
    uint32_t s;
    __host__ __device__ float u() {  // [0, 1)
        s = hash32(s);
        return (float)(s >> 8) * 0x1p-24f;
    }
    __host__ __device__ float sym() { return 2.0f * u() - 1.0f; }          // [-1, 1)
    __host__ __device__ float mag() {                                       // +-[0.5, 2)
        const float m = 0.5f + 1.5f * u();
        return u() < 0.5f ? -m : m;
    }
};
__host__ __device__ inline F3 unit(F3 v) {
    const float inv = 1.0f / sqrtf((v.x * v.x + v.y * v.y) + v.z * v.z);
    return F3{v.x * inv, v.y * inv, v.z * inv};
}
__host__ __device__ inline F3 rand_dir(Rng& r) {
    F3 v;
    do v = F3{r.sym(), r.sym(), r.sym()};
    while ((v.x * v.x + v.y * v.y) + v.z * v.z < 0.01f);
    return unit(v);
}
__host__ __device__ inline void set_sphere(Input& in, uint32_t k, float x, float y, float z, float r, float rr, uint32_t idx) {
    in.rec[4 * k + 0] = make_float4(x, y, z, r);
#ifdef __HIP_DEVICE_COMPILE__
    in.rec[4 * k + 1] = make_float4(rr, 0.0f, 0.0f, __uint_as_float(idx));
#else
    float f;
    std::memcpy(&f, &idx, 4);
    in.rec[4 * k + 1] = make_float4(rr, 0.0f, 0.0f, f);
#endif
}

// the input of index i; its kind is that of its wave
__host__ __device__ inline uint32_t kind_of(uint32_t i) { return (i / 64u) % kKinds; }
__host__ __device__ inline bool single_of(uint32_t i) { return ((i / 64u) / kKinds) % 2u == 1u; }
__host__ __device__ inline void make_input(uint32_t i, Input& in) {
    Rng r{hash32(i ^ 0x9e3779b9u)};
    const uint32_t kind = kind_of(i);
    // original indices: distinct, in no particular order (ties go to the lower one, not to the first tested)
    const uint32_t rot = hash32(i) % 3u;
    const uint32_t idx[3] = {2u + 3u * rot, 2u + 3u * ((rot + 1u) % 3u), 2u + 3u * ((rot + 2u) % 3u)};
    const float scale = kind == 3u || kind == 4u ? 0x1p-49f : (kind == 5u ? 0x1p26f : 1.0f);
    in.o = kind == 3u || kind == 4u ? F3{0.0f, 0.0f, 0.0f} : F3{scale * 2.0f * r.sym(), scale * 2.0f * r.sym(), scale * 2.0f * r.sym()};
    for (uint32_t k = 0; k < kNS; ++k) {
        const float rad = scale * (0.1f + 1.5f * r.u());
        set_sphere(in, k, scale * r.mag(), scale * r.mag(), scale * r.mag(), rad, rad * rad, idx[k]);
    }
    // aimed at a point of one sphere's box (three in four), away from it (one in four of those)
    const uint32_t aim = hash32(i + 77u) % 4u;
    in.d = rand_dir(r);
    if (aim < kNS) {
        const float4 s = in.rec[4 * aim];
        F3 v{(s.x + s.w * r.sym()) - in.o.x, (s.y + s.w * r.sym()) - in.o.y, (s.z + s.w * r.sym()) - in.o.z};
        if ((v.x * v.x + v.y * v.y) + v.z * v.z > 0.0f) in.d = unit(v);
        if (r.u() < 0.25f) in.d = F3{-in.d.x, -in.d.y, -in.d.z};
    }
    uint32_t keep = hash32(i / 64u) % kNS;  // (a wave of all-but-one spheres behind the ray keeps this one)
    if (kind == 2u) {  // 1e-4 off sphere 0 along its normal, leaving at a grazing angle; inside sphere 1
        const float4 s = in.rec[0];
        const F3 n = rand_dir(r);
        in.o = F3{(s.x + s.w * n.x) + 1e-4f * n.x, (s.y + s.w * n.y) + 1e-4f * n.y, (s.z + s.w * n.z) + 1e-4f * n.z};
        const F3 q = rand_dir(r);
        const F3 t = unit(cross3(n, F3{q.x + 0.01f, q.y, q.z + 0.02f}));
        const float e = 2e-3f * r.sym();
        in.d = unit(F3{t.x + e * n.x, t.y + e * n.y, t.z + e * n.z});
        const float r1 = 0.6f + 0.6f * r.u();
        set_sphere(in, 1, in.o.x + 0.3f * r.sym(), in.o.y + 0.3f * r.sym(), in.o.z + 0.3f * r.sym(), r1, r1 * r1, idx[1]);
        keep = 0u;
    } else if (kind == 4u) {  // crafted: d = (1/2, 1/2, 1/2), a = 3/4 and 4 a = 3 exactly
        in.d = F3{0.5f, 0.5f, 0.5f};
        const uint32_t j = i & 15u;
        const float sm = 0x1p-49f * (float)(1u + (hash32(i) & 7u));  // a few bits: its products are exact
        if (j < 9u) {  // the ray starts at the center: b = 0, c = -rr, disc = 3 rr within 4 ulps of 2^-96
            uint32_t u;
            const float rr0 = 0x1p-96f / 3.0f;
            std::memcpy(&u, &rr0, 4);
            u += j - 4u;
            float rr;
            std::memcpy(&rr, &u, 4);
            set_sphere(in, 0, 0.0f, 0.0f, 0.0f, 0x1p-48f, rr, idx[0]);
        } else if (j == 9u) {  // a point at the origin of the ray: b = c = disc = 0
            set_sphere(in, 0, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, idx[0]);
        } else if (j == 10u) {  // a point behind the ray, on its line: b = 3 s > 0, c = 3 s^2 > 0, disc = 0
            set_sphere(in, 0, -sm, -sm, -sm, 0.0f, 0.0f, idx[0]);
        } else if (j == 11u) {  // tangent: L = (s, -s, 0): b = 0, c = 2 s^2 - rr = 0, disc = 0
            set_sphere(in, 0, -sm, sm, 0.0f, sm, 2.0f * (sm * sm), idx[0]);
        } else {  // behind the ray on its line, a small radius: b > 0, c > 0 just under 3 s^2, disc > 0 small
            const float rad = sm * (0.01f + 0.5f * r.u());
            set_sphere(in, 0, -sm, -sm, -sm, rad, rad * rad, idx[0]);
        }
        keep = 0u;
    } else if (kind == 6u) {  // inside sphere 0 and a concentric sphere 1; sphere 2 = sphere 0 (another index)
        const float4 s = in.rec[0];
        in.o = F3{s.x + 0.3f * s.w * r.sym(), s.y + 0.3f * s.w * r.sym(), s.z + 0.3f * s.w * r.sym()};
        const float r1 = 0.7f * s.w;
        set_sphere(in, 1, s.x, s.y, s.z, r1, r1 * r1, idx[1]);
        set_sphere(in, 2, s.x, s.y, s.z, s.w, s.w * s.w, idx[2]);
    } else if (kind == 7u) {  // three unit spheres in a row along a line, the ray nearly along it
        const F3 l = rand_dir(r);
        for (uint32_t k = 0; k < kNS; ++k) {
            const float at = 2.0f + 2.5f * (float)k;
            set_sphere(in, k, in.o.x + at * l.x, in.o.y + at * l.y, in.o.z + at * l.z, 1.0f, 1.0f, idx[k]);
        }
        in.d = unit(F3{l.x + 0.2f * r.sym(), l.y + 0.2f * r.sym(), l.z + 0.2f * r.sym()});
    }
    if (single_of(i)) {  // every sphere but `keep` behind the ray, 3 radii back: b = 6 r a > 0, c = (9 a - 1) r^2 > 0
        for (uint32_t k = 0; k < kNS; ++k) {
            if (k == keep) continue;
            const float rad = kind == 4u || kind == 3u ? 0x1p-49f : in.rec[4 * k].w + (kind == 5u ? 1.0f : 0x1p-10f);
            const float back = 3.0f * rad;
            set_sphere(in, k, in.o.x - back * in.d.x, in.o.y - back * in.d.y, in.o.z - back * in.d.z, rad, rad * rad, idx[k]);
        }
    }
}

// stage 1 of one sphere, isect_sphere_fast's expressions
struct Stage1 {
    float b, c, disc;
};
__host__ __device__ inline Stage1 stage1(float4 s, float rr, F3 o, F3 d, float a) {
    const float lx = o.x - s.x, ly = o.y - s.y, lz = o.z - s.z;
    const float b = 2.0f * ((lx * d.x + ly * d.y) + lz * d.z);
    const float c = ((lx * lx + ly * ly) + lz * lz) - rr;
    return Stage1{b, c, b * b - 4.0f * a * c};
}
__host__ __device__ inline bool valid_disc(float disc) { return (disc >= 0x1p-96f) | (disc == 0.0f); }

enum { kBadCull, kBadKey3, kBadKey2, kBadRedo, kSecond, kSecond2, kHits, kCounters };

template <uint32_t kN>
__device__ __forceinline__ uint64_t loop_key(const float4* rec, F3 o, F3 d, float a, RcpRef r2a, uint64_t best, bool& redo) {
#pragma unroll
    for (uint32_t k = 0; k < kN; ++k) {
        const float t = isect_sphere_fast(rec[4 * k], rec[4 * k + 1].x, o, d, a, r2a, kTNear, redo);
        const uint64_t key = ((uint64_t)__float_as_uint(t) << 32) | __float_as_uint(rec[4 * k + 1].w);
        best = key < best ? key : best;
    }
    return best;
}

__global__ __launch_bounds__(256) void k_check(uint32_t n, unsigned long long* ctr, uint32_t* first_bad) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;  // (n is a multiple of 256: every lane of every wave runs)
    Input in;
    make_input(i, in);
    const float a = (in.d.x * in.d.x + in.d.y * in.d.y) + in.d.z * in.d.z;
    const RcpRef r2a = rcp_ref(2.0f * a);
    bool bad_cull = false;
    for (uint32_t k = 0; k < kNS; ++k) {
        const Stage1 s1 = stage1(in.rec[4 * k], in.rec[4 * k + 1].x, in.o, in.d, a);
        bool redo = false;
        const float t = isect_sphere_fast(in.rec[4 * k], in.rec[4 * k + 1].x, in.o, in.d, a, r2a, kTNear, redo);
        if (s1.b > 0.0f && s1.c > 0.0f && __float_as_uint(t) != __float_as_uint(kInf)) bad_cull = true;
    }
    // the search starts from a miss, or (one input in four) from a hit at a finite distance, as a shadow ray's does
    const float t0 = (hash32(i + 13u) & 3u) == 0u ? 3.0f * (i % 5u == 0u ? 0x1p-49f : 1.0f) : kInf;
    const uint64_t start = ((uint64_t)__float_as_uint(t0) << 32) | kMiss;
    bool redo_l3 = false, redo_l2 = false, redo_p3 = false, redo_p2 = false;
    const uint64_t want3 = loop_key<3>(in.rec, in.o, in.d, a, r2a, start, redo_l3);
    const uint64_t want2 = loop_key<2>(in.rec, in.o, in.d, a, r2a, start, redo_l2);
    __shared__ uint32_t s_second[4];  // [1]: flat_sphere_pass<3>'s second passes, [3]: flat_sphere_pass<2>'s
    if (threadIdx.x < 4u) s_second[threadIdx.x] = 0u;
    __syncthreads();
    uint64_t got3 = start, got2 = start;
    flat_sphere_pass<3>(in.rec, in.o, in.d, a, r2a, kTNear, redo_p3, got3, s_second);
    flat_sphere_pass<2>(in.rec, in.o, in.d, a, r2a, kTNear, redo_p2, got2, s_second + 2);
    // closest_flat's reading of the key: the starting hit if nothing beat it, and no index beside t = inf (the
    // index bits of a key with t = inf are those of whichever sphere or lane default came first: never read)
    auto hit = [&](uint64_t key) {
        const uint32_t tb = (uint32_t)(key >> 32);
        return key == start ? start : (((uint64_t)tb << 32) | (__uint_as_float(tb) < kInf ? (uint32_t)key : kMiss));
    };
    const bool bad3 = hit(got3) != hit(want3), bad2 = hit(got2) != hit(want2), bad_redo = redo_p3 != redo_l3 || redo_p2 != redo_l2;
    if (bad_cull) atomicAdd(&ctr[kBadCull], 1ull);
    if (bad3) atomicAdd(&ctr[kBadKey3], 1ull);
    if (bad2) atomicAdd(&ctr[kBadKey2], 1ull);
    if (bad_redo) atomicAdd(&ctr[kBadRedo], 1ull);
    if ((uint32_t)(want3 >> 32) != __float_as_uint(t0)) atomicAdd(&ctr[kHits], 1ull);
    if (bad_cull || bad3 || bad2 || bad_redo) atomicMin(first_bad, i);
    __syncthreads();
    if (threadIdx.x == 0u) {
        if (s_second[1]) atomicAdd(&ctr[kSecond], (unsigned long long)s_second[1]);
        if (s_second[3]) atomicAdd(&ctr[kSecond2], (unsigned long long)s_second[3]);
    }
    (void)n;
}

// --host: the inputs' coverage of the cases named above, per kind
struct Cover {
    unsigned long long n, culled, culled_valid, valid, zero, tiny, at_edge_lo, at_edge_hi, b_small, b_large, many, inside, single_many;
};

int host_coverage() {
    static const char* names[kKinds] = {"random", "random", "grazing", "size 2^-49", "crafted", "size 2^27", "duplicate", "in a row"};
    Cover tot{};
    bool ok = true;
    for (uint32_t kind = 0; kind < kKinds; ++kind) {
        Cover c{};
        for (uint32_t i = 0; i < kInputs; ++i) {
            if (kind_of(i) != kind) {
                i += 63u;  // (a wave is of one kind)
                continue;
            }
            Input in;
            make_input(i, in);
            const float a = (in.d.x * in.d.x + in.d.y * in.d.y) + in.d.z * in.d.z;
            if (!(a >= 0.5f && a <= 2.0f)) {
                std::printf("input %u: a = %g outside [0.5, 2]\n", i, a);
                return 1;
            }
            uint32_t cand = 0;
            for (uint32_t k = 0; k < kNS; ++k) {
                const Stage1 s = stage1(in.rec[4 * k], in.rec[4 * k + 1].x, in.o, in.d, a);
                const bool cull = s.b > 0.0f && s.c > 0.0f, v = valid_disc(s.disc);
                c.culled += cull;
                c.culled_valid += cull && v;
                c.valid += v;
                c.zero += s.disc == 0.0f;
                c.tiny += s.disc > 0.0f && s.disc < 0x1p-96f;
                c.at_edge_lo += s.disc >= 0x1p-96f * 0.999999f && s.disc < 0x1p-96f;
                c.at_edge_hi += s.disc >= 0x1p-96f && s.disc <= 0x1p-96f * 1.000001f;
                c.b_small += std::fabs(s.b) >= 0x1p-50f && std::fabs(s.b) <= 0x1p-46f;
                c.b_large += std::fabs(s.b) >= 0x1p28f;
                c.inside += v && s.c <= 0.0f;
                cand += v && !cull;
            }
            c.many += cand >= 2u;
            c.single_many += single_of(i) && cand >= 2u;
            ++c.n;
        }
        std::printf("%-10s %9llu inputs: culled %llu (valid disc %llu), valid %llu, disc = 0 %llu, 0 < disc < 2^-96 %llu, "
                    "within 1e-6 below / above 2^-96 %llu / %llu, |b| near 2^-48 %llu, |b| >= 2^28 %llu, origin in or on %llu, "
                    "two or more candidates %llu\n", names[kind], c.n, c.culled, c.culled_valid, c.valid, c.zero, c.tiny,
                    c.at_edge_lo, c.at_edge_hi, c.b_small, c.b_large, c.inside, c.many);
        ok = ok && c.single_many == 0ull;
        unsigned long long* t = &tot.n;
        const unsigned long long* s = &c.n;
        for (size_t f = 0; f < sizeof(Cover) / sizeof(unsigned long long); ++f) t[f] += s[f];
    }
    const bool reached = tot.culled_valid && tot.zero && tot.tiny && tot.at_edge_lo && tot.at_edge_hi && tot.b_small &&
                         tot.b_large && tot.many && tot.inside && tot.n == kInputs;
    if (!ok) std::printf("a wave meant to have one candidate per lane has a lane with two\n");
    if (!reached) std::printf("[a case is not reached]\n");
    std::printf("sphere cull: %llu inputs (host: not launched): %s\n", tot.n, ok && reached ? "PASS" : "FAIL");
    return ok && reached ? 0 : 1;
}

bool ck(hipError_t e, const char* what) {
    if (e == hipSuccess) return true;
    std::printf("HIP error: %s: %s\n", what, hipGetErrorString(e));
    return false;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc > 1 && std::strcmp(argv[1], "--host") == 0) return host_coverage();
    if (argc > 1) {
        std::printf("usage: test_sphere_cull [--host]\n");
        return 2;
    }
    unsigned long long* d_ctr = nullptr;
    uint32_t* d_first = nullptr;
    unsigned long long ctr[kCounters] = {};
    uint32_t first = 0xffffffffu;
    if (!ck(hipMalloc((void**)&d_ctr, sizeof ctr), "hipMalloc") || !ck(hipMalloc((void**)&d_first, 4), "hipMalloc") ||
        !ck(hipMemset(d_ctr, 0, sizeof ctr), "hipMemset") || !ck(hipMemcpy(d_first, &first, 4, hipMemcpyHostToDevice), "hipMemcpy"))
        return 1;
    static_assert(kInputs % 256u == 0u, "whole blocks");
    hipLaunchKernelGGL(k_check, dim3(kInputs / 256u), dim3(256), 0, 0, kInputs, d_ctr, d_first);
    if (!ck(hipGetLastError(), "k_check") || !ck(hipDeviceSynchronize(), "k_check") ||
        !ck(hipMemcpy(ctr, d_ctr, sizeof ctr, hipMemcpyDeviceToHost), "hipMemcpy") ||
        !ck(hipMemcpy(&first, d_first, 4, hipMemcpyDeviceToHost), "hipMemcpy"))
        return 1;
    (void)hipFree(d_ctr);
    (void)hipFree(d_first);
    const unsigned long long waves = kInputs / 64u;
    std::printf("sphere cull: %u inputs, %llu hits; culled spheres that returned a hit %llu; key mismatches %llu (3 spheres) "
                "%llu (2 spheres); redo mismatches %llu; second passes %llu (3 spheres) %llu (2 spheres) of %llu waves\n",
                kInputs, ctr[kHits], ctr[kBadCull], ctr[kBadKey3], ctr[kBadKey2], ctr[kBadRedo], ctr[kSecond], ctr[kSecond2], waves);
    if (first != 0xffffffffu) std::printf("first bad input: %u (kind %u)\n", first, kind_of(first));
    // every other group of eight waves has one candidate per lane at the most: no second pass there
    const bool both = ctr[kSecond] > 0ull && ctr[kSecond] <= waves / 2u && ctr[kSecond2] <= waves / 2u && ctr[kHits] > kInputs / 16u;
    const bool ok = !ctr[kBadCull] && !ctr[kBadKey3] && !ctr[kBadKey2] && !ctr[kBadRedo] && both;
    if (!both) std::printf("the second-pass counts or the hit count are outside what the inputs are built for\n");
    std::printf("%s\n", ok ? "PASS" : "FAIL");
    return ok ? 0 : 1;
}
