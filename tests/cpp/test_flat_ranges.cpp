// Host check of a flat scene's range predicate (scene.cpp flat_ranges_ok) and of its bit in the shape key
// (spt_kernels.h kShapeRanges, flat_ranges_baked, flat_tangent_baked): the Cornell box passes; each term of the
// predicate on both sides of its bound; the bit overlaps no other field of the key and counts only with a baked
// configuration of at most kRangesMaxBounces bounces; the tangent's form follows SPT_FLAG_ABS_FLOAT and the
// sphere count. Pure host code.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "scene.h"
#include "spt.h"
#include "spt_kernels.h"
#include "spt_launch_plan.h"

using namespace spt;

static int g_failed = 0;
#define CHECK(cond)                                                       \
    do {                                                                  \
        if (!(cond)) {                                                    \
            if (++g_failed <= 20) std::printf("line %d: %s\n", __LINE__, #cond); \
        }                                                                 \
    } while (0)

struct Scene {
    std::vector<spt_prim> prims;
    std::vector<spt_material> mats;
};

static Scene cornell() {
    Scene s;
    uint32_t n = 0, n_mats = 0;
    spt_env env;
    CHECK(spt_build_scene(SPT_SCENE_CORNELL, nullptr, &n, nullptr, &n_mats, nullptr) == SPT_OK);
    s.prims.resize(n);
    s.mats.resize(n_mats);
    CHECK(spt_build_scene(SPT_SCENE_CORNELL, s.prims.data(), &n, s.mats.data(), &n_mats, &env) == SPT_OK);
    return s;
}

static bool ranges(const Scene& s) {
    std::vector<DevPrim> dp;
    const char* msg = nullptr;
    if (!prepare_prims(s.prims.data(), (uint32_t)s.prims.size(), (uint32_t)s.mats.size(), dp, &msg)) {
        std::printf("prepare_prims: %s\n", msg ? msg : "?");
        ++g_failed;
        return false;
    }
    return flat_ranges_ok(s.prims.data(), (uint32_t)s.prims.size(), s.mats.data(), (uint32_t)s.mats.size(), dp);
}

static spt_prim sphere(float x, float y, float z, float r, uint32_t material) {
    spt_prim p{};
    p.type = SPT_PRIM_SPHERE;
    p.material = material;
    p.p0[0] = x; p.p0[1] = y; p.p0[2] = z; p.p0[3] = r;
    return p;
}
static spt_prim quad(const float q[3], const float u[3], const float v[3], uint32_t material) {
    spt_prim p{};
    p.type = SPT_PRIM_QUAD;
    p.material = material;
    for (int k = 0; k < 3; ++k) {
        p.p0[k] = q[k];
        p.p1[k] = u[k];
        p.p2[k] = v[k];
    }
    return p;
}

int main() {
    const Scene base = cornell();
    CHECK(ranges(base));
    {  // albedo: 0 and [2^-5, 1] pass, anything else fails
        const float ok[] = {0.0f, 0x1p-5f, 1.0f, 0.5f};
        const float bad[] = {0x1p-6f, std::nextafter(0x1p-5f, 0.0f), std::nextafter(1.0f, 2.0f), 1.5f, -0.5f, NAN, INFINITY};
        for (float a : ok) {
            Scene s = base;
            s.mats[0].albedo[1] = a;
            CHECK(ranges(s));
        }
        for (float a : bad) {
            Scene s = base;
            s.mats[0].albedo[1] = a;
            CHECK(!ranges(s));
        }
        // a zero in every channel of some material or other: the throughput can vanish, so no
        Scene s = base;
        s.mats[0].albedo[0] = 0.0f;
        s.mats[1].albedo[1] = 0.0f;
        CHECK(ranges(s));  // (blue is nonzero throughout)
        s.mats[2].albedo[2] = 0.0f;
        CHECK(!ranges(s));
    }
    {  // emission: >= +0 with the sign bit clear
        const float ok[] = {0.0f, 1e-45f, 15.0f, INFINITY};
        const float bad[] = {-0.0f, -1.0f, NAN};
        for (float e : ok) {
            Scene s = base;
            s.mats[3].emission[2] = e;
            CHECK(ranges(s));
        }
        for (float e : bad) {
            Scene s = base;
            s.mats[3].emission[2] = e;
            CHECK(!ranges(s));
        }
    }
    {  // spheres: r * r in [2^-90, 2^90] and r >= E / 32 (Cornell's coordinate bound E is 8: the back wall's z)
        Scene s = base;
        s.prims.push_back(sphere(0.0f, 0.0f, 5.0f, 0x1p-46f, 0));
        CHECK(!ranges(s));
        s.prims.back() = sphere(0.0f, 0.0f, 5.0f, 0.25f, 0);  // 8 / 32
        CHECK(ranges(s));
        s.prims.back() = sphere(0.0f, 0.0f, 5.0f, std::nextafter(0.25f, 0.0f), 0);
        CHECK(!ranges(s));
        // alone, at its own scale: the window's two ends, and one step past each
        Scene t;
        t.mats = base.mats;
        t.prims = {sphere(0.0f, 0.0f, 0.0f, 0x1p-45f, 0)};
        CHECK(ranges(t));
        t.prims = {sphere(0.0f, 0.0f, 0.0f, 0x1p-46f, 0)};
        CHECK(!ranges(t));
        t.prims = {sphere(0.0f, 0.0f, 0.0f, 0x1p27f, 0)};
        CHECK(ranges(t));
        t.prims = {sphere(0.0f, 0.0f, 0.0f, 0x1p28f, 0)};  // past fast_division_ok
        CHECK(!ranges(t));
    }
    {  // stored normals: the squared length's window, and a scene past fast_division_ok's bound
        const float q[3] = {0.0f, 0.0f, 5.0f};
        Scene t;
        t.mats = base.mats;
        const float u1[3] = {0x1p-23f, 0.0f, 0.0f}, v1[3] = {0.0f, 0x1p-23f, 0.0f};  // |n|^2 = 2^-92
        t.prims = {quad(q, u1, v1, 0)};
        CHECK(!ranges(t));
        const float u2[3] = {0x1p-22f, 0.0f, 0.0f}, v2[3] = {0.0f, 0x1p-23f, 0.0f};  // 2^-90
        t.prims = {quad(q, u2, v2, 0)};
        CHECK(ranges(t));
        const float u3[3] = {0x1p23f, 0.0f, 0.0f}, v3[3] = {0.0f, 0x1p23f, 0.0f};  // 2^92
        t.prims = {quad(q, u3, v3, 0)};
        CHECK(!ranges(t));
        Scene s = base;
        s.prims[0].p0[0] = 0x1p28f;
        CHECK(!ranges(s));
    }
    {  // the key's bit: alone in its place, and what the kernels make of it
        const uint64_t plain = flat_shape_key(0x3fffffffu, 63u, 7u, 63u), with = flat_shape_key(0x3fffffffu, 63u, 7u, 63u, true);
        CHECK((plain >> 63) == 0 && with == (plain | kShapeRanges));
        CHECK(flat_shape_key(1u, 2u, 3u, 4u, false) == flat_shape_key(1u, 2u, 3u, 4u));
        CHECK(flat_shape_pairs(with) == flat_shape_pairs(plain) && flat_pair_table_bytes(with) == flat_pair_table_bytes(plain));
        const uint64_t all = jit_config_key(plain, 63u, 63u, 1u, kFlagAbsFloatBit | kFlagFastDiv, true);
        CHECK((all & kShapeRanges) == 0);  // no other field reaches bit 63
        // a key without the configuration, or with more than kRangesMaxBounces bounces, runs the guarded forms
        const uint64_t two = flat_shape_key(2u, 8u, 7u, 5u, true), none = flat_shape_key(0u, 6u, 7u, 5u, true);
        CHECK(!flat_ranges_baked(two));
        for (uint32_t b = 0; b < 64u; ++b) {
            CHECK(flat_ranges_baked(jit_config_key(two, b, 2u, 1u, kFlagFastDiv)) == (b <= kRangesMaxBounces));
            CHECK(!flat_ranges_baked(jit_config_key(flat_shape_key(2u, 8u, 7u, 5u), b, 2u, 1u, kFlagFastDiv)));
        }
        CHECK(kRangesMaxBounces == 9u);  // (2^-5)^(9 - 1) = 2^-40, div_ref's smallest divisor
        // the tangent: with SPT_FLAG_ABS_FLOAT, or in a shape without spheres
        CHECK(!flat_tangent_baked(jit_config_key(two, 8u, 2u, 1u, kFlagFastDiv)));
        CHECK(flat_tangent_baked(jit_config_key(two, 8u, 2u, 1u, kFlagFastDiv | kFlagAbsFloatBit)));
        CHECK(flat_tangent_baked(jit_config_key(none, 8u, 2u, 1u, kFlagFastDiv)));
        CHECK(!flat_tangent_baked(jit_config_key(none, 10u, 2u, 1u, kFlagFastDiv)));
        // the bit names another kernel: the same form, another shape argument
        const PathsVariant timed{false, false, 0, 0, false, 0};
        CHECK(jit_form(timed, with) == jit_form(timed, plain));
        CHECK(jit_name_expr(jit_form(timed, with), with) != jit_name_expr(jit_form(timed, plain), plain));
    }
    if (g_failed) {
        std::printf("%d check(s) failed\n", g_failed);
        return 1;
    }
    std::printf("flat ranges ok\n");
    return 0;
}
