// Host check of a context's cached-state record (spt_ctx_state.h DerivedState): what each change drops. The
// matrix below is written out from the code before the record existed — it is the statement of that behaviour,
// not a copy of the header's table. spt_launch_plan.h is included for frame_hit_mode alone.
#include <cstdio>

#include "spt_ctx_state.h"
#include "spt_launch_plan.h"

using namespace spt;

static int g_failed = 0;
#define CHECK(cond)                                                       \
    do {                                                                  \
        if (!(cond)) {                                                    \
            if (++g_failed <= 20) std::printf("line %d: %s\n", __LINE__, #cond); \
        }                                                                 \
    } while (0)

static const Derived kItems[9] = {kCameraHits, kChunkOrder, kViewLists, kFeatures, kDenoised,
                                  kCapturedView, kHistory, kBlended, kReusable};
static const Change kCauses[10] = {Change::Scene, Change::Prims, Change::Configuration, Change::Buffers, Change::Sky,
                                   Change::Camera, Change::Lens, Change::Materials, Change::Counters, Change::HistoryClear};
// kDropped[cause][item], items in kItems' order: 1 = the cause drops the item
static const int kDropped[10][9] = {
    // hits order view  feat  dn  capt  hist blend reus
    {1, 1, 1, 1, 0, 1, 1, 0, 1},  // Scene
    {1, 1, 1, 1, 0, 1, 1, 0, 0},  // Prims
    {1, 1, 1, 1, 1, 1, 1, 1, 0},  // Configuration
    {1, 1, 1, 1, 1, 1, 1, 1, 0},  // Buffers
    {0, 0, 1, 0, 0, 1, 1, 0, 0},  // Sky
    {1, 1, 1, 1, 0, 0, 1, 0, 0},  // Camera
    {1, 1, 1, 0, 0, 0, 1, 0, 0},  // Lens
    {1, 1, 1, 0, 0, 1, 1, 0, 1},  // Materials
    {1, 0, 1, 0, 0, 0, 0, 0, 0},  // Counters
    {0, 0, 0, 0, 0, 1, 1, 0, 0},  // HistoryClear
};

constexpr uint64_t kKey = 0x8000000000001234ull, kKeyA = 77u, kKeyB = 99u;

// item i made valid the way its producer does
static void produce(DerivedState& s, int i) {
    switch (kItems[i]) {
        case kCameraHits: s.produced_camera_hits(true); break;
        case kChunkOrder: s.chunk_order_key = kKey; break;  // (the launch writes it through the pointer it takes)
        case kViewLists: s.produced_view_lists(); break;
        case kDenoised: s.produced_denoised(1); break;
        default: s.produced(kItems[i]);
    }
}

static bool same(const DerivedState& a, const DerivedState& b) {
    return a.bits == b.bits && a.chunk_order_key == b.chunk_order_key && a.half_order_key[0] == b.half_order_key[0] &&
           a.half_order_key[1] == b.half_order_key[1] && a.dn_result == b.dn_result;
}

int main() {
    static_assert(sizeof(kDrops) / sizeof(kDrops[0]) == 10, "ten causes");
    DerivedState fresh;
    for (int i = 0; i < 9; ++i) CHECK(!fresh.valid(kItems[i]));
    CHECK(!fresh.frame_lists() && !fresh.valid(kViewNoMemory) && fresh.dn_result == -1);

    for (int c = 0; c < 10; ++c) {
        // the matrix: from everything valid
        DerivedState all;
        for (int i = 0; i < 9; ++i) produce(all, i);
        all.half_order_key[0] = kKeyA;
        all.half_order_key[1] = kKeyB;
        all.produced(kViewNoMemory);
        for (int i = 0; i < 9; ++i) CHECK(all.valid(kItems[i]));
        CHECK(all.frame_lists() && all.dn_result == 1);
        DerivedState s = all;
        s.drop(kCauses[c]);
        for (int i = 0; i < 9; ++i) CHECK(s.valid(kItems[i]) == !kDropped[c][i]);
        // the lists go with the hits; a non-zero key goes to 0 or stays as it was; the image index likewise
        CHECK(s.frame_lists() == !kDropped[c][0]);
        CHECK(s.chunk_order_key == (kDropped[c][1] ? 0u : kKey));
        CHECK(s.dn_result == (kDropped[c][4] ? -1 : 1));
        // the halves' keys and the failed allocation go with the buffers alone
        const bool buffers = kCauses[c] == Change::Buffers;
        CHECK(s.half_order_key[0] == (buffers ? 0u : kKeyA) && s.half_order_key[1] == (buffers ? 0u : kKeyB));
        CHECK(s.valid(kViewNoMemory) == !buffers);
        // idempotence
        DerivedState twice = s;
        twice.drop(kCauses[c]);
        CHECK(same(twice, s));
        // from one item valid: a drop never validates anything
        for (int only = 0; only < 9; ++only) {
            DerivedState one;
            produce(one, only);
            one.drop(kCauses[c]);
            for (int i = 0; i < 9; ++i) CHECK(one.valid(kItems[i]) == (i == only && !kDropped[c][i]));
            CHECK(!one.valid(kViewNoMemory) && one.half_order_key[0] == 0u && one.half_order_key[1] == 0u);
            CHECK(one.frame_lists() == (only == 0 && !kDropped[c][0]));
        }
    }

    // camera hits: none / hits / hits and lists, seen through frame_hit_mode (a pinhole, no material models)
    PassParams p{};
    DerivedState h;
    CHECK(frame_hit_mode(p, h.valid(kCameraHits), h.frame_lists()) == 1u);
    h.produced_camera_hits(false);
    CHECK(h.valid(kCameraHits) && !h.frame_lists());
    CHECK(frame_hit_mode(p, h.valid(kCameraHits), h.frame_lists()) == 2u);
    h.produced_camera_hits(true);
    CHECK(frame_hit_mode(p, h.valid(kCameraHits), h.frame_lists()) == 3u);
    h.produced_camera_hits(false);  // (hits stored again without lists: the lists are not kept)
    CHECK(frame_hit_mode(p, h.valid(kCameraHits), h.frame_lists()) == 2u);
    for (int c = 0; c < 10; ++c) {
        DerivedState s;
        s.produced_camera_hits(true);
        s.drop(kCauses[c]);
        CHECK(s.valid(kCameraHits) || !s.frame_lists());  // never lists without hits
        CHECK(frame_hit_mode(p, s.valid(kCameraHits), s.frame_lists()) == (kDropped[c][0] ? 1u : 3u));
    }

    // view lists: producing them zeroes both halves' keys and leaves the whole view's alone
    DerivedState v;
    v.chunk_order_key = kKey;
    v.half_order_key[0] = kKeyA;
    v.half_order_key[1] = kKeyB;
    v.produced_view_lists();
    CHECK(v.valid(kViewLists) && v.half_order_key[0] == 0u && v.half_order_key[1] == 0u && v.chunk_order_key == kKey);

    // clear before the launch, set after: begin() drops the one item and nothing else
    for (int i = 0; i < 9; ++i) {
        DerivedState s;
        for (int k = 0; k < 9; ++k) produce(s, k);
        s.begin(kItems[i]);
        for (int k = 0; k < 9; ++k) CHECK(s.valid(kItems[k]) == (k != i));
        produce(s, i);
        CHECK(s.valid(kItems[i]));
    }
    DerivedState d;
    d.produced_denoised(0);
    CHECK(d.valid(kDenoised) && d.dn_result == 0);

    if (g_failed == 0) std::puts("ctx state ok");
    return g_failed ? 1 : 0;
}
