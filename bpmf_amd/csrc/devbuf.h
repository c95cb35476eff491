// devbuf.h -- owning device and pinned allocations of the add-ons of a side (ext_state.h): freed when they go out of scope, counted
// while they live.  Included by state.h behind fail() and HIP_TRY, which report the errors (BPMF_HIP_ENOMEM / BPMF_HIP_ENODEV, as
// dev_upload).  The caller has set the device.
#pragma once
#include <utility>

// live DevBuf / Pinned allocations of the process and the device bytes of the former (bpmf_hip_live_device_bytes): hipMemGetInfo
// counts the whole card, other processes included
inline std::atomic<int64_t> g_live_allocs{0}, g_live_bytes{0};
// host waits for a context's main stream so far in this process (bounded_stream_sync; bpmf_hip_stream_drains): what a loop that
// claims not to drain must leave unchanged
inline std::atomic<int64_t> g_stream_drains{0};

template <typename T>
class DevBuf {
    T *p_ = nullptr;
    size_t bytes_ = 0;

public:
    DevBuf() = default;
    DevBuf(DevBuf &&o) noexcept : p_(std::exchange(o.p_, nullptr)), bytes_(std::exchange(o.bytes_, 0)) {}
    DevBuf &operator=(DevBuf &&o) noexcept { std::swap(p_, o.p_); std::swap(bytes_, o.bytes_); return *this; }   // (o frees what this held)
    ~DevBuf() { reset(); }

    T *get() const { return p_; }
    explicit operator bool() const { return p_ != nullptr; }
    void reset()
    {
        if (!p_) return;
        (void)hipFree(p_);
        g_live_allocs.fetch_sub(1, std::memory_order_relaxed);
        g_live_bytes.fetch_sub((int64_t)bytes_, std::memory_order_relaxed);
        p_ = nullptr; bytes_ = 0;
    }
    // n elements, uninitialised (n = 0: one element, so that a live buffer is never NULL)
    int alloc(size_t n)
    {
        reset();
        const size_t bytes = std::max<size_t>(n, 1) * sizeof(T);
        const hipError_t e = hipMalloc((void **)&p_, bytes);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            p_ = nullptr;
            return fail(e == hipErrorOutOfMemory ? BPMF_HIP_ENOMEM : BPMF_HIP_ENODEV,
                        "hipMalloc of " + std::to_string(bytes) + " bytes: " + hipGetErrorString(e));
        }
        bytes_ = bytes;
        g_live_allocs.fetch_add(1, std::memory_order_relaxed);
        g_live_bytes.fetch_add((int64_t)bytes, std::memory_order_relaxed);
        return 0;
    }
    int upload(const T *src, size_t n)
    {
        const int rc = alloc(n);
        if (rc) return rc;
        if (src && n) HIP_TRY(hipMemcpy(p_, src, n * sizeof(T), hipMemcpyHostToDevice));
        return 0;
    }
    int zero_async(hipStream_t st) { HIP_TRY(hipMemsetAsync(p_, 0, bytes_, st)); return 0; }
};

// n elements of mapped pinned host memory and their address on the device (host memory: no part of the live bytes)
template <typename T>
class Pinned {
    T *h_ = nullptr, *d_ = nullptr;

public:
    Pinned() = default;
    Pinned(Pinned &&o) noexcept : h_(std::exchange(o.h_, nullptr)), d_(std::exchange(o.d_, nullptr)) {}
    Pinned &operator=(Pinned &&o) noexcept { std::swap(h_, o.h_); std::swap(d_, o.d_); return *this; }
    ~Pinned() { reset(); }

    T *host() const { return h_; }
    T *dev() const { return d_; }
    explicit operator bool() const { return h_ != nullptr; }
    void reset()
    {
        if (!h_) return;
        (void)hipHostFree(h_);
        g_live_allocs.fetch_sub(1, std::memory_order_relaxed);
        h_ = d_ = nullptr;
    }
    int alloc(size_t n)
    {
        reset();
        HIP_TRY(hipHostMalloc((void **)&h_, n * sizeof(T), hipHostMallocMapped));
        g_live_allocs.fetch_add(1, std::memory_order_relaxed);
        HIP_TRY(hipHostGetDevicePointer((void **)&d_, h_, 0));
        return 0;
    }
};
