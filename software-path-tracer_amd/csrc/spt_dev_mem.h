// spt_dev_mem.h — the owner of one device allocation: a pointer, its element count, freed when the owner goes.
// A context (spt_capi.hip spt_ctx) keeps every device buffer in one of these, grouped into records by what frees
// them (the scene's, the configuration's, the context's own), so dropping a record frees its buffers and no list
// of them is kept by hand. Alloc is the allocator: two static functions, void* alloc(size_t bytes) (nullptr: no
// memory) and void free(void*); spt_capi.hip's calls hipMalloc / hipFree, tests/cpp/test_dev_mem.cpp's malloc /
// free. Pure host code, no HIP. Internal.
#pragma once

#include <cstddef>
#include <cstdint>

namespace spt {

template <class T, class Alloc>
class DevBuf {
public:
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept { swap(o); }
    DevBuf& operator=(DevBuf&& o) noexcept {  // (what this held is freed here, not with o)
        if (this != &o) {
            reset();
            swap(o);
        }
        return *this;
    }
    ~DevBuf() { reset(); }

    void reset() {
        if (p_) Alloc::free(p_);
        p_ = nullptr;
        n_ = 0;
    }
    void swap(DevBuf& o) noexcept {
        T* p = p_;
        const size_t n = n_;
        p_ = o.p_;
        n_ = o.n_;
        o.p_ = p;
        o.n_ = n;
    }

    // Exactly n elements, uninitialized; what was held is freed first. false: no memory, or n * sizeof(T) does
    // not fit a size_t — the buffer is then empty. n == 0: empty, true.
    bool alloc(size_t n) {
        reset();
        if (n == 0) return true;
        if (n > SIZE_MAX / sizeof(T)) return false;
        p_ = static_cast<T*>(Alloc::alloc(n * sizeof(T)));
        if (!p_) return false;
        n_ = n;
        return true;
    }
    // an allocation of exactly n elements is kept, contents and all; any other is replaced as alloc(n) does
    bool ensure(size_t n) { return n_ == n || alloc(n); }
    // ... of at least n elements (scratch that only grows)
    bool ensure_at_least(size_t n) { return n_ >= n || alloc(n); }

    size_t size() const { return n_; }  // elements
    operator T*() const { return p_; }  // (no operator bool: `!buf`, `buf + k` and a T* parameter take this one)

private:
    T* p_ = nullptr;
    size_t n_ = 0;
};

}  // namespace spt
