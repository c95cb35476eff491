// devbuf.h -- the owners of everything the library holds on the device: device buffers (DevBuf), mapped pinned host memory (Pinned),
// events (Event) and streams (Stream), each released when it goes out of scope.  The add-ons of a side (ext_state.h) and the core
// state behind the handles (state.h: context, side, test set) are owned the same way; no other file allocates or releases.
// Device bytes are counted while they live, in two counters: the add-ons' DevBuf<T> into g_live_bytes (bpmf_hip_live_device_bytes),
// the core state's DevBuf<T, true> into g_core_bytes (bpmf_hip_live_core_bytes) -- the core state of a side is built lazily by
// its first bpmf_hip_sys_sample, which must not move the add-ons' counter.  Included by state.h behind fail() and HIP_TRY, which
// report the errors (BPMF_HIP_ENOMEM / BPMF_HIP_ENODEV).  The caller has set the device.
#pragma once
#include <utility>

// device bytes of the live DevBuf allocations of the process, add-ons / core state: hipMemGetInfo counts the whole card, other
// processes included
inline std::atomic<int64_t> g_live_bytes{0}, g_core_bytes{0};
// host waits for a context's main stream so far in this process (bounded_stream_sync; bpmf_hip_stream_drains): what a loop that
// claims not to drain must leave unchanged
inline std::atomic<int64_t> g_stream_drains{0};

template <typename T, bool Core = false>
class DevBuf {
    T *p_ = nullptr;
    size_t bytes_ = 0;
    static std::atomic<int64_t> &counter() { return Core ? g_core_bytes : g_live_bytes; }

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
        counter().fetch_sub((int64_t)bytes_, std::memory_order_relaxed);
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
        counter().fetch_add((int64_t)bytes, std::memory_order_relaxed);
        return 0;
    }
    int upload(const T *src, size_t n)
    {
        const int rc = alloc(n);
        if (rc) return rc;
        if (src && n) HIP_TRY(hipMemcpy(p_, src, n * sizeof(T), hipMemcpyHostToDevice));
        return 0;
    }
    int zero() { HIP_TRY(hipMemset(p_, 0, bytes_)); return 0; }
    int zero_async(hipStream_t st) { HIP_TRY(hipMemsetAsync(p_, 0, bytes_, st)); return 0; }
};

// n elements of mapped pinned host memory and their address on the device (host memory: counted by neither counter)
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
        h_ = d_ = nullptr;
    }
    int alloc(size_t n)
    {
        reset();
        HIP_TRY(hipHostMalloc((void **)&h_, n * sizeof(T), hipHostMallocMapped));
        HIP_TRY(hipHostGetDevicePointer((void **)&d_, h_, 0));
        return 0;
    }
};

// the core state's device buffers (state.h)
template <typename T>
using CoreBuf = DevBuf<T, true>;

class Event {
    hipEvent_t ev_ = nullptr;

public:
    Event() = default;
    Event(Event &&o) noexcept : ev_(std::exchange(o.ev_, nullptr)) {}
    Event &operator=(Event &&o) noexcept { std::swap(ev_, o.ev_); return *this; }
    ~Event() { reset(); }

    hipEvent_t get() const { return ev_; }
    explicit operator bool() const { return ev_ != nullptr; }
    void reset()
    {
        if (ev_) (void)hipEventDestroy(ev_);
        ev_ = nullptr;
    }
    int create(unsigned flags = hipEventDefault)
    {
        reset();
        HIP_TRY(hipEventCreateWithFlags(&ev_, flags));
        return 0;
    }
};

// The device time of a span of a stream between two events, created on first use.  begin / end record around the launches; resolve,
// after the host has waited for the stream, reads the time.  ms < 0: nothing has been timed, or the time could not be read.
struct Timed {
    Event ev[2];
    float ms = -1.f;
    int begin(hipStream_t st)
    {
        for (Event &e : ev) if (!e) { const int rc = e.create(); if (rc) return rc; }
        ms = -1.f;
        HIP_TRY(hipEventRecord(ev[0].get(), st));
        return 0;
    }
    int end(hipStream_t st) { HIP_TRY(hipEventRecord(ev[1].get(), st)); return 0; }
    void resolve()
    {
        if (hipEventElapsedTime(&ms, ev[0].get(), ev[1].get()) != hipSuccess) { (void)hipGetLastError(); ms = -1.f; }
    }
};

// a stream of the library's own, or the caller's (borrow: never destroyed here)
class Stream {
    hipStream_t s_ = nullptr;
    bool owned_ = false;

public:
    Stream() = default;
    Stream(Stream &&o) noexcept : s_(std::exchange(o.s_, nullptr)), owned_(std::exchange(o.owned_, false)) {}
    Stream &operator=(Stream &&o) noexcept { std::swap(s_, o.s_); std::swap(owned_, o.owned_); return *this; }
    ~Stream() { reset(); }

    hipStream_t get() const { return s_; }
    explicit operator bool() const { return s_ != nullptr; }
    void reset()
    {
        if (s_ && owned_) (void)hipStreamDestroy(s_);
        s_ = nullptr; owned_ = false;
    }
    void borrow(hipStream_t s) { reset(); s_ = s; }
    int create(unsigned flags)
    {
        reset();
        HIP_TRY(hipStreamCreateWithFlags(&s_, flags));
        owned_ = true;
        return 0;
    }
    int create(unsigned flags, int priority)
    {
        reset();
        HIP_TRY(hipStreamCreateWithPriority(&s_, flags, priority));
        owned_ = true;
        return 0;
    }
};
