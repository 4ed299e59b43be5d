// cm_devbuf.hpp — the one place where the library takes and gives back memory of its own: DevBuf<T> owns one hipMalloc
// allocation, PinnedBuf<T> one hipHostMalloc allocation, and each remembers its capacity in elements (DevBuf<void>: in bytes).
// Every owned buffer of the context is one of the two (cm_ctx.hpp), so a destroyed context gives back what it took without a
// list of its fields, and a by-product that needs a buffer adds a field and nothing else.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <type_traits>
#include <utility>

#ifdef CM_TEST_HOOKS                     // (the test build only: allocations alive in the process, and made so far)
#include <atomic>
#include <cstdint>
inline std::atomic<uint64_t> cm_allocations_live{0}, cm_allocations_total{0};
#endif

// bytes of HBM (pinned: of page-locked host memory), or nullptr: HIP's sticky error is cleared here, so that a later
// hipGetLastError() does not report an out-of-memory that was handled.
inline void* cm_take(size_t bytes, bool pinned) {
    void* p = nullptr;
    const hipError_t e = pinned ? hipHostMalloc(&p, bytes, hipHostMallocDefault) : hipMalloc(&p, bytes);
    if (e != hipSuccess || !p) { (void)hipGetLastError(); return nullptr; }
#ifdef CM_TEST_HOOKS
    ++cm_allocations_live;
    ++cm_allocations_total;
#endif
    return p;
}

inline void cm_give(void* p, bool pinned) {
    if (!p) return;
    (void)(pinned ? hipHostFree(p) : hipFree(p));
#ifdef CM_TEST_HOOKS
    --cm_allocations_live;
#endif
}

template <class T, bool Pinned = false>
class DevBuf {
    static constexpr size_t elem = sizeof(std::conditional_t<std::is_void<T>::value, char, T>);
    T* p_ = nullptr;
    size_t cap_ = 0;

public:
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p_(std::exchange(o.p_, nullptr)), cap_(std::exchange(o.cap_, 0)) {}
    DevBuf& operator=(DevBuf&& o) noexcept { std::swap(p_, o.p_); std::swap(cap_, o.cap_); return *this; }
    ~DevBuf() { release(); }

    operator T*() const { return p_; }   // launches and pointer arithmetic read as with a plain pointer
    T* operator->() const { return p_; }
    size_t capacity() const { return cap_; }

    // Room for n elements: nothing happens when n fits; otherwise the old allocation is freed first and exactly n are
    // allocated (contents are never kept, old and new never live at once). false: out of memory, the buffer is empty.
    bool reserve(size_t n) {
        if (n <= cap_) return true;
        release();
        p_ = static_cast<T*>(cm_take(n * elem, Pinned));
        cap_ = p_ ? n : 0;
        return p_ != nullptr;
    }
    // n elements on the first call, nothing afterwards: a buffer of one size for the context's life.
    bool once(size_t n) { return p_ || reserve(n); }
    void release() {
        cm_give(p_, Pinned);
        p_ = nullptr;
        cap_ = 0;
    }
};

template <class T> using PinnedBuf = DevBuf<T, true>;
