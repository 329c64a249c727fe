// DevBuf (csrc/spt_dev_mem.h), the owner of one device allocation, over a host allocator that counts: malloc / free,
// the blocks alive, the requests made, and a request that can be told to fail. No GPU, no HIP header. Built and
// run by tests/test_dev_mem_host.py, once plainly and once under the address and undefined-behaviour sanitizers
// (a double free or a use of a freed block stops that run; a leak is the live count below). Prints one line.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <utility>

#include "spt_dev_mem.h"

namespace {

struct HostAlloc {
    static int live, requests, fail_at;  // fail_at: the request (counted from 1) that returns nullptr, 0: none
    static void* alloc(size_t bytes) {
        if (++requests == fail_at) return nullptr;
        void* p = std::malloc(bytes);
        if (p) {
            std::memset(p, 0xa5, bytes);  // (every byte asked for is there to write)
            ++live;
        }
        return p;
    }
    static void free(void* p) {
        --live;
        std::free(p);
    }
    static void fail_next() { fail_at = requests + 1; }
};
int HostAlloc::live = 0, HostAlloc::requests = 0, HostAlloc::fail_at = 0;

template <class T>
using Buf = spt::DevBuf<T, HostAlloc>;

int failures = 0;
#define CHECK(cond)                                                       \
    do {                                                                  \
        if (!(cond)) {                                                    \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);         \
            ++failures;                                                   \
        }                                                                 \
    } while (0)

struct Wide {
    float v[4];
};

void takes_pointer(const Wide* p, const Wide* want) { CHECK(p == want); }

void test_alloc() {
    Buf<Wide> b;
    CHECK(b.size() == 0 && !b && b == nullptr && HostAlloc::live == 0);
    CHECK(b.alloc(7) && b.size() == 7 && b && HostAlloc::live == 1);
    Wide* const first = b;
    first[6].v[3] = 1.0f;  // the last element is inside the block (the sanitizer run checks it)
    takes_pointer(b, first);
    CHECK(b + 2 == first + 2);
    CHECK(b.alloc(3) && b.size() == 3 && HostAlloc::live == 1);  // the old block went, exactly 3 came
    CHECK(b.alloc(0) && b.size() == 0 && !b && HostAlloc::live == 0);
    const int before = HostAlloc::requests;
    CHECK(b.alloc(0) && HostAlloc::requests == before);  // nothing is asked of the allocator for 0 elements
    b.reset();
    b.reset();  // (an empty buffer's reset does nothing)
    CHECK(HostAlloc::live == 0);
}

void test_ensure() {
    Buf<uint32_t> b;
    CHECK(b.ensure(5) && b.size() == 5);
    uint32_t* const first = b;
    first[4] = 77u;
    const int before = HostAlloc::requests;
    CHECK(b.ensure(5) && b == first && first[4] == 77u && HostAlloc::requests == before);  // equal: kept, contents too
    CHECK(b.ensure(6) && b.size() == 6 && HostAlloc::requests == before + 1 && HostAlloc::live == 1);  // larger: replaced
    CHECK(b.ensure(2) && b.size() == 2 && HostAlloc::requests == before + 2 && HostAlloc::live == 1);  // smaller: replaced
    CHECK(b.ensure(0) && b.size() == 0 && !b && HostAlloc::live == 0);
    // at least n: a larger or equal one is kept, a smaller one replaced by exactly n
    CHECK(b.ensure_at_least(4) && b.size() == 4);
    uint32_t* const kept = b;
    const int mid = HostAlloc::requests;
    CHECK(b.ensure_at_least(4) && b.ensure_at_least(1) && b.ensure_at_least(0) && b == kept && b.size() == 4);
    CHECK(HostAlloc::requests == mid);
    CHECK(b.ensure_at_least(9) && b.size() == 9 && HostAlloc::requests == mid + 1 && HostAlloc::live == 1);
}

void test_failure() {
    Buf<Wide> b;
    CHECK(b.alloc(4) && HostAlloc::live == 1);
    HostAlloc::fail_next();
    CHECK(!b.alloc(8) && b.size() == 0 && !b && HostAlloc::live == 0);  // empty, the old block freed
    CHECK(b.alloc(4) && HostAlloc::live == 1);                            // ... and usable again
    HostAlloc::fail_next();
    CHECK(!b.ensure(5) && b.size() == 0 && !b && HostAlloc::live == 0);
    CHECK(b.ensure(4));
    HostAlloc::fail_next();
    CHECK(!b.ensure_at_least(5) && b.size() == 0 && !b && HostAlloc::live == 0);
    HostAlloc::fail_at = 0;
    // n * sizeof(T) beyond size_t: a failure, and the allocator is never asked (for a wrapped, small size)
    CHECK(b.alloc(2));
    const int before = HostAlloc::requests;
    CHECK(!b.alloc(SIZE_MAX / sizeof(Wide) + 1) && b.size() == 0 && !b && HostAlloc::live == 0);
    CHECK(!b.ensure(SIZE_MAX) && !b.ensure_at_least(SIZE_MAX / 2) && HostAlloc::requests == before);
    Buf<uint8_t> bytes;  // (sizeof 1: every count fits, and the largest is the allocator's to refuse)
    HostAlloc::fail_next();
    CHECK(!bytes.alloc(SIZE_MAX) && HostAlloc::requests == before + 1 && HostAlloc::live == 0);
    HostAlloc::fail_at = 0;
}

void test_move_and_swap() {
    Buf<uint32_t> a, b;
    CHECK(a.alloc(3) && b.alloc(5) && HostAlloc::live == 2);
    uint32_t* const pa = a;
    uint32_t* const pb = b;
    a.swap(b);
    CHECK(a == pb && a.size() == 5 && b == pa && b.size() == 3 && HostAlloc::live == 2);
    Buf<uint32_t> c(std::move(a));  // move construction: the source is empty
    CHECK(c == pb && c.size() == 5 && !a && a.size() == 0 && HostAlloc::live == 2);
    b = std::move(c);  // move assignment: the target's block is freed, the source is empty
    CHECK(b == pb && b.size() == 5 && !c && c.size() == 0 && HostAlloc::live == 1);
    Buf<uint32_t>& self = b;
    b = std::move(self);  // onto itself: unchanged
    CHECK(b == pb && b.size() == 5 && HostAlloc::live == 1);
    CHECK(a.alloc(1) && HostAlloc::live == 2);  // a moved-from buffer is an empty one: usable
    {
        Buf<uint32_t> local;  // the allocate-then-swap-in pattern: the old block leaves with the local
        CHECK(local.alloc(8));
        b.swap(local);
        CHECK(HostAlloc::live == 3);
    }
    CHECK(b.size() == 8 && HostAlloc::live == 2);
}

struct Record {  // as spt_ctx's records: several owners, arrays of them, and a nested struct
    Buf<Wide> image, pair[2];
    Buf<uint32_t> words;
    struct {
        Buf<uint16_t> cost;
    } half[2];
    Buf<float> never;  // (stays empty)
};

void test_record() {
    Record r;
    CHECK(r.image.alloc(4) && r.pair[0].alloc(2) && r.pair[1].alloc(2) && r.words.alloc(9) && r.half[0].cost.alloc(1) &&
          r.half[1].cost.alloc(1));
    CHECK(HostAlloc::live == 6);
    r = {};  // each block freed exactly once (twice would stop the sanitizer run, and take live below 0)
    CHECK(HostAlloc::live == 0);
    CHECK(!r.image && !r.pair[0] && !r.pair[1] && !r.words && !r.half[0].cost && !r.half[1].cost && !r.never);
    r = {};
    CHECK(HostAlloc::live == 0);
    CHECK(r.image.ensure(3) && r.half[1].cost.ensure(2) && HostAlloc::live == 2);  // and the record goes on being used
}  // (its destructor frees the two)

}  // namespace

int main() {
    static_assert(!std::is_copy_constructible<Buf<float>>::value && !std::is_copy_assignable<Buf<float>>::value, "move-only");
    static_assert(std::is_convertible<Buf<float>, float*>::value && !std::is_convertible<Buf<float>, uint32_t*>::value,
                  "a buffer converts to its own pointer type");
    test_alloc();
    CHECK(HostAlloc::live == 0);
    test_ensure();
    CHECK(HostAlloc::live == 0);
    test_failure();
    CHECK(HostAlloc::live == 0);
    test_move_and_swap();
    CHECK(HostAlloc::live == 0);
    test_record();
    CHECK(HostAlloc::live == 0);
    if (failures) return 1;
    std::printf("dev mem ok\n");
    return 0;
}
