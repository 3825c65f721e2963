// owned.hpp — the small owning helpers every handle of the host side is built from: what a handle or a feature
// allocates is made on one line and given back by release().  Host only: the device translation units never see
// this file.  None of them synchronises behind the caller's back, except where its comment says so.
#pragma once
#include <vector>

#include "internal.hpp"

// returns the status of a call that failed (it has set the error text)
#define CSIM_TRY(expr)           \
    do {                         \
        int rc_ = (expr);        \
        if (rc_) return rc_;     \
    } while (0)

namespace csim {

// the array of T that starts `byte` bytes into a buffer (the layouts of obs_taps.hpp give the offsets)
template <class T> T* buf_at(void* base, size_t byte) { return reinterpret_cast<T*>(static_cast<char*>(base) + byte); }

// A device buffer, made on first use and grown to the largest request.  reserve: a buffer that is large enough is
// untouched; one that is too small is replaced, after `idle` (if given) has drained, since work enqueued there may
// still use the old one.  A failed allocation leaves the buffer absent (cap 0), and the next call tries again.
struct DeviceBuf {
    void* p = nullptr;
    size_t cap = 0;  // bytes
    template <class T = double> T* as() const { return static_cast<T*>(p); }
    int reserve(size_t bytes, hipStream_t idle = nullptr) {
        if (bytes <= cap) return CSIM_OK;
        if (idle) CSIM_HIP(hipStreamSynchronize(idle));
        release();
        CSIM_HIP(hipMalloc(&p, bytes));
        cap = bytes;
        return CSIM_OK;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr, cap = 0;
    }
};

// The same in pinned host memory; the owner sees to it that no copy still uses a buffer that is replaced.
struct PinnedBuf {
    void* p = nullptr;
    size_t cap = 0;  // bytes
    template <class T = double> T* as() const { return static_cast<T*>(p); }
    int reserve(size_t bytes) {
        if (bytes <= cap) return CSIM_OK;
        release();
        CSIM_HIP(hipHostMalloc(&p, bytes, hipHostMallocDefault));
        cap = bytes;
        return CSIM_OK;
    }
    void release() {
        if (p) (void)hipHostFree(p);
        p = nullptr, cap = 0;
    }
};

// The result of a diagnostic kernel and its way to the host (the _begin / _wait pairs, csim_stepper_snapshot_begin
// among them): the kernel runs in stream order on the owner's stream (the sweeps after it write the other ping-pong
// buffer first, and never `dev`), and only the copy to the pinned buffer goes to `io`, so the next run does not wait
// for it.  Every kind of capture has a Capture, and so a copy stream, of its own: none waits for another kind's copy.
struct Capture {
    DeviceBuf dev;
    PinnedBuf host;
    hipStream_t io = nullptr;   // non-blocking, carries the copies to `host`
    hipEvent_t done = nullptr;  // the kernel that wrote `dev` has run
    bool pending = false;       // a copy to `host` is in flight or waits to be fetched
    // Before the kernel is enqueued: lets a copy in flight finish (it reads `dev`) and makes room for `bytes`, in
    // `host` too when the call is a _begin.  `idle` as in DeviceBuf::reserve.  A replaced pinned buffer has nothing
    // to fetch any more.
    int prepare(size_t bytes, bool pinned, hipStream_t idle) {
        if (!io) CSIM_HIP(hipStreamCreateWithFlags(&io, hipStreamNonBlocking));
        if (!done) CSIM_HIP(hipEventCreateWithFlags(&done, hipEventDisableTiming));
        if (pending) CSIM_HIP(hipStreamSynchronize(io));
        CSIM_TRY(dev.reserve(bytes, idle));
        if (!pinned || bytes <= host.cap) return CSIM_OK;
        pending = false;
        return host.reserve(bytes);
    }
    // after the kernel: `bytes` of `dev` to `host` on `io`, once everything enqueued on `st` so far is done
    int begin(size_t bytes, hipStream_t st) {
        CSIM_HIP(hipEventRecord(done, st));
        CSIM_HIP(hipStreamWaitEvent(io, done, 0));
        CSIM_HIP(hipMemcpyAsync(host.p, dev.p, bytes, hipMemcpyDeviceToHost, io));
        pending = true;
        return CSIM_OK;
    }
    int wait(const char* none_in_flight) {
        if (!pending) return fail(CSIM_ERR_STATE, none_in_flight);
        CSIM_HIP(hipStreamSynchronize(io));
        pending = false;
        return CSIM_OK;
    }
    void release() {
        if (io) (void)hipStreamSynchronize(io);
        dev.release();
        host.release();
        if (done) (void)hipEventDestroy(done);
        if (io) (void)hipStreamDestroy(io);
        done = nullptr, io = nullptr, pending = false;
    }
};

// A host input on its way to the device, copied before the call returns: host -> pinned staging -> device, in stream
// order.
struct Staging {
    PinnedBuf host;
    hipEvent_t copied = nullptr;  // the last copy out of `host` has run
    bool used = false;
    // *h: room for `bytes`, to be filled by the caller, once the last copy out of the buffer has run (the event is
    // made here, at the first input that is staged)
    int acquire(size_t bytes, void** h) {
        if (!copied) CSIM_HIP(hipEventCreateWithFlags(&copied, hipEventDisableTiming));
        if (used) CSIM_HIP(hipEventSynchronize(copied));
        used = false;
        CSIM_TRY(host.reserve(bytes));
        *h = host.p;
        return CSIM_OK;
    }
    int send(void* dst, size_t bytes, hipStream_t st) {
        CSIM_HIP(hipMemcpyAsync(dst, host.p, bytes, hipMemcpyHostToDevice, st));
        CSIM_HIP(hipEventRecord(copied, st));
        used = true;
        return CSIM_OK;
    }
    void release() {
        host.release();
        if (copied) (void)hipEventDestroy(copied);
        copied = nullptr, used = false;
    }
};

// What a handle makes when it is created and keeps until it is destroyed: device buffers of a fixed size, streams and
// events.  Each is made by one call here, which hands out a raw view (the pointer the launches and RCCL read, the
// hipStream_t, the hipEvent_t) and records it; release() gives back whatever was made, so a create that fails half-way
// and a destroy are the same call and nothing is listed twice.  One hipMalloc per buffer: no arena.
struct Owned {
    std::vector<DeviceBuf> mem;
    std::vector<hipEvent_t> events;
    std::vector<hipStream_t> streams;
    Owned() = default;
    Owned(const Owned&) = delete;
    Owned& operator=(const Owned&) = delete;
    ~Owned() { release(); }
    // `bytes` of device memory, zero-filled on the null stream when asked
    template <class T> int device(T** view, size_t bytes, bool zeroed = false) {
        DeviceBuf b;
        CSIM_TRY(b.reserve(bytes));
        mem.push_back(b);
        *view = b.as<T>();
        if (zeroed) CSIM_HIP(hipMemset(b.p, 0, bytes));
        return CSIM_OK;
    }
    // memory that came from another allocator call and goes back through hipFree (signal memory)
    void adopt(void* p, size_t bytes) { mem.push_back(DeviceBuf{p, bytes}); }
    int event(hipEvent_t* view, unsigned flags = hipEventDisableTiming) {
        CSIM_HIP(hipEventCreateWithFlags(view, flags));
        events.push_back(*view);
        return CSIM_OK;
    }
    // a non-blocking stream; high: of the device's highest priority
    int stream(hipStream_t* view, bool high = false) {
        int lo = 0, hi = 0;  // numerically lower = higher priority
        if (high) CSIM_HIP(hipDeviceGetStreamPriorityRange(&lo, &hi));
        CSIM_HIP(high ? hipStreamCreateWithPriority(view, hipStreamNonBlocking, hi)
                      : hipStreamCreateWithFlags(view, hipStreamNonBlocking));
        streams.push_back(*view);
        return CSIM_OK;
    }
    // host wait for every stream made here (errors ignored: this is the way out)
    void drain() const {
        for (hipStream_t st : streams) (void)hipStreamSynchronize(st);
    }
    // memory, then events, then streams; the views the handle keeps are dead afterwards
    void release() {
        for (DeviceBuf& b : mem) b.release();
        for (hipEvent_t ev : events) (void)hipEventDestroy(ev);
        for (hipStream_t st : streams) (void)hipStreamDestroy(st);
        mem.clear(), events.clear(), streams.clear();
    }
};

}  // namespace csim
