// Host check of the opposite wall pairs of a flat scene's kind-major copy (scene.cpp flat_wall_pairs) and
// of their bits in the shape key (spt_kernels.h flat_shape_key): Cornell's pairs, nested pairs, coplanar
// quads, a group that is not all rectangles, every record kept exactly once, the lower plane first in
// each pair, and the key's round trip. Pure host code (also built with -fsanitize=address,undefined).
#include <algorithm>
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

static uint32_t f2u(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}

static spt_prim quad(float qx, float qy, float qz, float ux, float uy, float uz, float vx, float vy, float vz) {
    spt_prim p{};
    p.type = SPT_PRIM_QUAD;
    p.p0[0] = qx; p.p0[1] = qy; p.p0[2] = qz;
    p.p1[0] = ux; p.p1[1] = uy; p.p1[2] = uz;
    p.p2[0] = vx; p.p2[1] = vy; p.p2[2] = vz;
    return p;
}
// a 2 x 2 wall on the plane x = at (edges along y and z)
static spt_prim wall_x(float at) { return quad(at, -1.f, 4.f, 0.f, 2.f, 0.f, 0.f, 0.f, 2.f); }

struct Sorted {
    std::vector<DevPrim> before, after;
    uint32_t ends[kFlatKinds - 1];
    uint32_t rect = 0, pairs = 0;
};

static bool prepare(const std::vector<spt_prim>& prims, Sorted& s) {
    std::vector<DevPrim> dp;
    const char* msg = nullptr;
    if (!prepare_prims(prims.data(), (uint32_t)prims.size(), 1, dp, &msg)) {
        std::printf("prepare_prims: %s\n", msg ? msg : "?");
        return false;
    }
    sort_flat_by_kind(dp, s.before, s.ends);
    s.rect = flat_rect_bits(s.before, s.ends);
    s.after = s.before;
    s.pairs = flat_wall_pairs(s.after, s.ends, s.rect);
    return true;
}

static uint32_t pairs_of(const Sorted& s, int ax) { return (s.pairs >> (2 * ax)) & 3u; }

// every record of every group kept exactly once (records outside the axis groups untouched), each pair's
// lower plane first and strictly below the higher one, pairs outermost first, no pair left among the rest
static void invariants(const Sorted& s) {
    CHECK(s.after.size() == s.before.size());
    const uint32_t n = (uint32_t)s.before.size();
    for (uint32_t k = 0; k < n; ++k) {
        const bool in_axis_group = k >= s.ends[0] && k < s.ends[3];
        if (!in_axis_group) CHECK(std::memcmp(&s.after[k], &s.before[k], sizeof(DevPrim)) == 0);
    }
    for (int ax = 0; ax < 3; ++ax) {
        const uint32_t b = s.ends[ax], e = s.ends[ax + 1], np = pairs_of(s, ax);
        CHECK(np <= kFlatMaxPairs && 2u * np <= e - b);
        if (!((s.rect >> ax) & 1u)) CHECK(np == 0);
        std::vector<uint32_t> ib, ia;  // the original indices (b.w): the same multiset, each once
        for (uint32_t k = b; k < e; ++k) {
            ib.push_back(f2u(s.before[k].b[3]));
            ia.push_back(f2u(s.after[k].b[3]));
        }
        std::sort(ib.begin(), ib.end());
        std::sort(ia.begin(), ia.end());
        CHECK(ib == ia);
        CHECK(std::adjacent_find(ia.begin(), ia.end()) == ia.end());
        for (uint32_t k = b; k < e; ++k) {  // whole records, not only the index
            bool found = false;
            for (uint32_t j = b; j < e; ++j) found = found || std::memcmp(&s.after[k], &s.before[j], sizeof(DevPrim)) == 0;
            CHECK(found);
        }
        for (uint32_t p = 0; p < np; ++p) {
            const float lo = s.after[b + 2 * p].a[ax], hi = s.after[b + 2 * p + 1].a[ax];
            CHECK(lo < hi);
            if (p > 0) {  // nested inside the pair before
                CHECK(s.after[b + 2 * p - 2].a[ax] <= lo);
                CHECK(hi <= s.after[b + 2 * p - 1].a[ax]);
            }
            for (uint32_t k = b + 2 * np; k < e; ++k) {  // the unpaired lie between the pairs' planes
                CHECK(lo <= s.after[k].a[ax]);
                CHECK(s.after[k].a[ax] <= hi);
            }
        }
        if (np < kFlatMaxPairs && ((s.rect >> ax) & 1u)) {  // what is left holds no two different planes
            for (uint32_t k = b + 2 * np; k < e; ++k) CHECK(s.after[k].a[ax] == s.after[b + 2 * np].a[ax]);
        }
    }
}

int main() {
    {  // Cornell: x one pair; y one pair (floor, ceiling) and the light unpaired; z none
        uint32_t n = 0, n_mats = 0;
        spt_env env;
        CHECK(spt_build_scene(SPT_SCENE_CORNELL, nullptr, &n, nullptr, &n_mats, nullptr) == SPT_OK);
        std::vector<spt_prim> prims(n);
        std::vector<spt_material> mats(n_mats);
        CHECK(spt_build_scene(SPT_SCENE_CORNELL, prims.data(), &n, mats.data(), &n_mats, &env) == SPT_OK);
        for (auto& p : prims) p.material = 0;
        Sorted s;
        CHECK(prepare(prims, s));
        invariants(s);
        CHECK(s.rect == 7u);
        CHECK(pairs_of(s, 0) == 1 && pairs_of(s, 1) == 1 && pairs_of(s, 2) == 0);
        CHECK(s.after[s.ends[0]].a[0] == -2.5f && s.after[s.ends[0] + 1].a[0] == 2.5f);
        CHECK(s.after[s.ends[1]].a[1] == -2.5f && s.after[s.ends[1] + 1].a[1] == 2.5f);
        CHECK(s.after[s.ends[1] + 2].a[1] == 2.495f);  // the light
        CHECK(s.ends[2] - s.ends[1] == 3u);
        // the key round-trips, and without pairs it is the key from before the pairs existed
        uint32_t fe = 0;
        for (uint32_t g = 0; g + 1 < kFlatKinds; ++g) fe |= s.ends[g] << (6 * g);
        const uint64_t key = flat_shape_key(fe, n, s.rect, s.pairs);
        CHECK(flat_shape_pairs(key, 0) == 1 && flat_shape_pairs(key, 1) == 1 && flat_shape_pairs(key, 2) == 0);
        CHECK(flat_shape_pairs(key) == 2);
        CHECK((key & ~(63ull << 57)) == flat_shape_key(fe, n, s.rect));
        CHECK(flat_shape_key(fe, n, s.rect, 0u) == flat_shape_key(fe, n, s.rect));
        CHECK(flat_shape_key(fe, n, s.rect) == 77445755138ull + (7ull << 53));
        CHECK(flat_pair_table_bytes(key) == 2u * 64u + 16u && flat_pair_table_bytes(flat_shape_key(fe, n, s.rect)) == 0u);
        // the launch configuration's bits do not overlap the pairs'
        const uint64_t cfg = jit_config_key(key, 63u, 63u, 1u, kFlagAbsFloatBit | kFlagFastDiv, true);
        CHECK(flat_shape_pairs(cfg, 0) == 1 && flat_shape_pairs(cfg, 1) == 1 && flat_shape_pairs(cfg, 2) == 0);
        CHECK((cfg >> 63) == 0);
        // the counting k_paths of a shape with pairs is compiled for the shape (it counts the second passes of
        // the test the timed kernel runs); without pairs the offline counting kernels run, as before
        const PathsVariant counting{true, false, 0, 0, false, 0}, counting_nee{true, false, 2, 0, false, kNeeAll};
        const PathsVariant timed{false, false, 0, 0, false, 0};
        CHECK(jit_form(counting, key) == jit_form_of(counting) && jit_form(counting_nee, key) == jit_form_of(counting_nee));
        CHECK(jit_form(counting, flat_shape_key(fe, n, s.rect)) == kNoJitForm);
        CHECK(jit_form(counting_nee, flat_shape_key(fe, n, s.rect)) == kNoJitForm);
        CHECK(jit_form(timed, key) == jit_form_of(timed));
        CHECK(jit_name_expr(jit_form(PathsVariant{true, false, 1, 0, false, 0}, key), 5ull) ==
              "spt::k_paths<true, false, 1, 5ull, 0, false, 0, false, false, false>");
        // (the NEE form's sky kind is 2 whatever the variant says)
        CHECK(jit_name_expr(jit_form(PathsVariant{true, false, 0, 0, false, kNeeAll}, key), 5ull) ==
              "spt::k_paths<true, false, 2, 5ull, 0, false, 1, false, false, false>");
        CHECK(jit_name_expr(jit_form(PathsVariant{false, false, 1, 0, false, 0}, key), 5ull) ==
              "spt::k_paths<false, false, 1, 5ull, 0, false, 0, false, false, false>");
        for (uint32_t pb = 0; pb < 64; ++pb) {
            const uint64_t k2 = flat_shape_key(fe, n, s.rect, pb);
            CHECK(flat_shape_pairs(k2, 0) == (pb & 3u) && flat_shape_pairs(k2, 1) == ((pb >> 2) & 3u) &&
                  flat_shape_pairs(k2, 2) == (pb >> 4));
        }
    }
    {  // four walls on x: two nested pairs, the outer (-3, 3) first, then (-1, 2)
        Sorted s;
        CHECK(prepare({wall_x(2.f), wall_x(-3.f), wall_x(3.f), wall_x(-1.f)}, s));
        invariants(s);
        CHECK(pairs_of(s, 0) == 2 && pairs_of(s, 1) == 0 && pairs_of(s, 2) == 0);
        const uint32_t b = s.ends[0];
        CHECK(s.after[b].a[0] == -3.f && s.after[b + 1].a[0] == 3.f && s.after[b + 2].a[0] == -1.f && s.after[b + 3].a[0] == 2.f);
    }
    {  // eight walls: three pairs at the most, the two innermost stay unpaired, in their earlier order
        Sorted s;
        CHECK(prepare({wall_x(1.f), wall_x(-4.f), wall_x(4.f), wall_x(-3.f), wall_x(3.f), wall_x(-2.f), wall_x(2.f), wall_x(-1.f)}, s));
        CHECK(pairs_of(s, 0) == 3);
        const uint32_t b = s.ends[0];
        CHECK(s.after[b + 6].a[0] == 1.f && s.after[b + 7].a[0] == -1.f);
        CHECK(f2u(s.after[b + 6].b[3]) == 0u && f2u(s.after[b + 7].b[3]) == 7u);
    }
    {  // coplanar quads are never paired; with a third plane only the two different planes are
        Sorted s;
        CHECK(prepare({wall_x(1.f), wall_x(1.f)}, s));
        invariants(s);
        CHECK(s.pairs == 0);
        Sorted t;
        CHECK(prepare({wall_x(1.f), wall_x(1.f), wall_x(-1.f)}, t));
        invariants(t);
        CHECK(pairs_of(t, 0) == 1);
        CHECK(t.after[t.ends[0]].a[0] == -1.f && t.after[t.ends[0] + 1].a[0] == 1.f && t.after[t.ends[0] + 2].a[0] == 1.f);
        Sorted u;  // -1, 1, 1, 1: one pair, and the rest all on one plane
        CHECK(prepare({wall_x(1.f), wall_x(1.f), wall_x(-1.f), wall_x(1.f)}, u));
        invariants(u);
        CHECK(pairs_of(u, 0) == 1);
    }
    {  // a group with a quad that is not a rectangle along the axes: no rect bit, no pairs, nothing moved
        Sorted s;
        CHECK(prepare({wall_x(-1.f), quad(1.f, -1.f, 4.f, 0.f, 2.f, 1.f, 0.f, 0.f, 2.f)}, s));
        invariants(s);
        CHECK((s.rect & 1u) == 0u && s.pairs == 0u);
        CHECK(std::memcmp(s.after.data(), s.before.data(), sizeof(DevPrim) * s.before.size()) == 0);
    }
    {  // a single wall, and an empty scene's groups
        Sorted s;
        CHECK(prepare({wall_x(1.f)}, s));
        invariants(s);
        CHECK(s.pairs == 0u);
    }
    if (g_failed) {
        std::printf("%d check(s) failed\n", g_failed);
        return 1;
    }
    std::printf("wall pairs ok\n");
    return 0;
}
