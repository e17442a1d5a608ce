// The scaffold of the synchronous host entries (numpy in, numpy out, on the NULL stream); bfgx_api.hip includes it before the first of them.
// An entry reads: argument checks, HostCall, buffers, ready(), work, finish().  Needs fail, HIP_TRY, select_device and DevBuf.
#pragma once
namespace {

// Selects the device, owns the device buffers of one call (one allocation each, released at scope exit on every return path) and copies
// the results back.  Failure is sticky: without a device, and after the first failed allocation or copy, every later request does nothing
// and returns nullptr, and ready() / finish() return that first failure; an entry reads `rc` itself only where it returns early for an
// empty input.  `count` is in elements; an empty request still gets a valid pointer (dev_malloc).
struct HostCall {
    int rc;                                                      // of the device selection, then of the first failed request
    explicit HostCall(int device) : rc(select_device(device)) {}
    HostCall(const HostCall &) = delete;
    HostCall &operator=(const HostCall &) = delete;
    ~HostCall() { while (!bufs.empty()) bufs.pop_back(); }       // newest first

    // allocated and filled from `host` (a NULL `host` uploads nothing)
    template <typename T> const T *in(const T *host, size_t count) { return (const T *)buffer(sizeof(T) * count, host, nullptr); }
    // allocated only
    template <typename T> T *scratch(size_t count) { return (T *)buffer(sizeof(T) * count, nullptr, nullptr); }
    // allocated; finish() copies it to `host` (a NULL `host`, an optional result, is not copied)
    template <typename T> T *out(T *host, size_t count) { return (T *)buffer(sizeof(T) * count, nullptr, host); }
    // filled from `host`, and copied back to it by finish()
    template <typename T> T *inout(T *host, size_t count) { return (T *)buffer(sizeof(T) * count, host, host); }
    // filled from `from`, and copied to `to` (which may be `from`) by finish(): an operation that works in place on the device
    template <typename T> T *inout(const T *from, T *to, size_t count) { return (T *)buffer(sizeof(T) * count, from, to); }

    int ready() const { return rc; }

    // the launches' status, then the results in the order they were requested (blocking copies: the NULL stream has drained when it returns)
    int finish()
    {
        if (rc) return rc;
        HIP_TRY(hipGetLastError());
        for (const Download &d : downloads) HIP_TRY(hipMemcpy(d.host, d.dev, d.bytes, hipMemcpyDeviceToHost));
        return BFGX_OK;
    }

private:
    struct Download { void *host; const void *dev; size_t bytes; };
    std::vector<DevBuf> bufs;
    std::vector<Download> downloads;

    void *buffer(size_t bytes, const void *src, void *dst)
    {
        if (rc) return nullptr;
        DevBuf b;
        if (hipError_t e = b.up(src, bytes)) {
            rc = fail(BFGX_ERR_HIP, "device buffer of %zu bytes: allocation or upload failed (%s)", bytes, hipGetErrorString(e));
            return nullptr;
        }
        if (dst) downloads.push_back({dst, b.p, bytes});
        bufs.push_back(std::move(b));
        return bufs.back().p;
    }
};

}  // namespace
