// bfgx_devmem.hpp -- device memory of libbfgx (host code only).  Device memory is allocated and freed only in this file: one counted
// allocation function and three owners.  None of them selects a device or waits for a stream (PoolBuf's growth excepted): whoever
// releases memory selects its device and drains the streams that may still read it first.  Page-locked host memory is not handled here.
//   DevBuf    one allocation, released at scope exit
//   PoolBuf   one grow-only allocation that outlives the call (the one-shot caches)
//   DevList   the allocations of a plan, released together
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>
#include <cstddef>
#include <type_traits>
#include <vector>

namespace bfgx {

// every device allocation the library makes is counted (bfgx_debug_alloc_count): a warm one-shot call must make none
inline std::atomic<long long> g_dev_allocs{0};
// ... and those not yet freed (bfgx_debug_live_allocs): what a handle allocated, its `end` gives back
inline std::atomic<long long> g_dev_live{0};

// the message of a failed allocation: fail(BFGX_ERR_HIP, kDevAllocFailed, "catalog")
constexpr const char *kDevAllocFailed = "hipMalloc(%s) failed";

// (an empty request still gets a distinct, valid pointer)
inline hipError_t dev_malloc(void **p, size_t bytes)
{
    ++g_dev_allocs;
    const hipError_t e = hipMalloc(p, bytes ? bytes : 8);
    if (e == hipSuccess) ++g_dev_live;
    return e;
}
inline void dev_free(void *p) { if (p) { --g_dev_live; (void)hipFree(p); } }

struct DevBuf {
    void *p = nullptr;
    DevBuf() = default;
    DevBuf(DevBuf &&o) noexcept : p(o.p) { o.p = nullptr; }
    DevBuf &operator=(DevBuf &&o) noexcept { if (this != &o) { dev_free(p); p = o.p; o.p = nullptr; } return *this; }
    ~DevBuf() { dev_free(p); }
    hipError_t alloc(size_t bytes) { dev_free(p); p = nullptr; return dev_malloc(&p, bytes); }
    // allocate, then copy `bytes` from the host (synchronous) if there is something to copy
    hipError_t up(const void *host, size_t bytes)
    {
        if (hipError_t e = alloc(bytes)) return e;
        return host && bytes ? hipMemcpy(p, host, bytes, hipMemcpyHostToDevice) : hipSuccess;
    }
    template <typename T> T *as() const { return (T *)p; }
};

// A grow-only device buffer: a request beyond its capacity reallocates it with a slack of bytes / div + add, after the device has
// drained (an earlier call may still use the old buffer on another stream).  Only growth waits; a warm call finds the buffer large enough.
struct PoolBuf {
    void *p = nullptr;
    size_t cap = 0;
    PoolBuf() = default;
    PoolBuf(const PoolBuf &) = delete;
    PoolBuf &operator=(const PoolBuf &) = delete;
    ~PoolBuf() { dev_free(p); }
    int need(size_t bytes, size_t div = 4, size_t add = 256)
    {
        if (bytes <= cap) return 0;
        if (p) { (void)hipDeviceSynchronize(); dev_free(p); }
        p = nullptr; cap = 0;
        const size_t want = bytes + bytes / div + add;
        if (dev_malloc(&p, want) != hipSuccess) { p = nullptr; return 1; }
        cap = want;
        return 0;
    }
    template <typename T> T *as() const { return (T *)p; }
};

struct DevList {
    std::vector<void *> v;
    DevList() = default;
    DevList(const DevList &) = delete;
    DevList &operator=(const DevList &) = delete;
    ~DevList() { release(); }
    void release() { for (void *d : v) dev_free(d); v.clear(); }
    // `count` elements of T; `out` is written on success only
    template <typename T> hipError_t alloc(T *&out, size_t count)
    {
        void *d = nullptr;
        if (hipError_t e = dev_malloc(&d, sizeof(T) * count)) return e;
        v.push_back(d);
        out = (T *)d;
        return hipSuccess;
    }
    // `count` elements of T filled from the host on a stream (the host array must outlive the copy)
    template <typename T> hipError_t upload(const T *&out, const T *host, size_t count, hipStream_t s)
    {
        T *d = nullptr;
        if (hipError_t e = alloc(d, count)) return e;
        out = d;
        return hipMemcpyAsync(d, host, sizeof(T) * count, hipMemcpyHostToDevice, s);
    }
    // replaces the allocation at `ptr` by a larger one (contents are not kept) and frees the old one at once: the caller has drained its stream
    template <typename T> hipError_t regrow(T *&ptr, size_t count)
    {
        void *d = nullptr;
        if (hipError_t e = dev_malloc(&d, sizeof(T) * count)) return e;
        for (void *&o : v) if (o == (void *)ptr) { dev_free(o); o = d; }
        ptr = (T *)d;
        return hipSuccess;
    }
};

static_assert(!std::is_copy_constructible<DevBuf>::value && !std::is_copy_constructible<PoolBuf>::value &&
              !std::is_copy_constructible<DevList>::value, "owners of device memory are not copyable");

}  // namespace bfgx
