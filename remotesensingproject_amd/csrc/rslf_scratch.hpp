// The one owning buffer type of the library: a pointer and a capacity in bytes that only ever grows.  Host-only like
// rslf_plan.hpp -- no HIP include, no device qualifier -- so it compiles with g++ alone and is unit-tested on the CPU under
// AddressSanitizer / UBSan with a counting allocator (tests/cpp/test_scratch.cpp, tests/test_plan_cpu.py).  The real
// allocators (device memory, pinned host memory) are the two policies in rslf_internal.hpp.
#pragma once

#include <stddef.h>

#include <utility>

namespace rslf {

// What GrowBuf::reserve reports: the allocator's error code (0 = none) and whether the caller has to fill the storage.
struct Reserved {
    int err;
    bool fresh;   // newly allocated, or marked stale since the last reserve.  A fill that later calls rely on covers all of
                  // capacity(), not the bytes asked for: kept storage may be larger, and a later, larger request that still
                  // fits is not fresh
};

// Alloc: a policy with `static int alloc(size_t bytes, void** out)` and `static int free(void* p)`, 0 = success.
template <typename Alloc>
class GrowBuf {
public:
    GrowBuf() = default;
    GrowBuf(const GrowBuf&) = delete;
    GrowBuf& operator=(const GrowBuf&) = delete;
    GrowBuf(GrowBuf&& o) noexcept : p_(o.p_), cap_(o.cap_), stale_(o.stale_) { o.forget(); }
    GrowBuf& operator=(GrowBuf&& o) noexcept
    {
        if (this != &o) {
            release();
            p_ = o.p_, cap_ = o.cap_, stale_ = o.stale_;
            o.forget();
        }
        return *this;
    }
    ~GrowBuf() { release(); }   // a failed free is not reported here

    // At least `bytes` of storage.  Enough already: nothing happens (the contents stay).  Else the old storage is freed
    // FIRST and the new allocated second: the peak footprint stays at the larger of the two, and with a device allocator the
    // free is what waits for work in flight on the memory being replaced.  A failed free leaves the buffer as it was; a
    // failed allocation leaves it empty, and the next reserve tries again.
    Reserved reserve(size_t bytes)
    {
        if (bytes <= cap_)
            return Reserved{0, std::exchange(stale_, false)};
        if (p_) {
            if (const int e = Alloc::free(p_))
                return Reserved{e, false};
            forget();
        }
        void* q = nullptr;
        if (const int e = Alloc::alloc(bytes, &q))
            return Reserved{e, false};
        p_ = q, cap_ = bytes;
        return Reserved{0, true};
    }

    // The contents can no longer be trusted: the storage is kept, and the next reserve reports it as fresh.
    void mark_stale() { stale_ = p_ != nullptr; }

    void release()
    {
        if (p_)
            (void)Alloc::free(p_);
        forget();
    }

    void* get() const { return p_; }
    template <typename T>
    T* as() const { return static_cast<T*>(p_); }
    size_t capacity() const { return cap_; }   // bytes

private:
    void forget() { p_ = nullptr, cap_ = 0, stale_ = false; }
    void* p_ = nullptr;
    size_t cap_ = 0;
    bool stale_ = false;
};

}  // namespace rslf
