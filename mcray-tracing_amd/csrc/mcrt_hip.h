// mcrt_hip.h -- host side only: the status macros and the owners of HIP resources that the context (mcrt_ctx.h: mcrt_api.cpp,
// mcrt_trace.cpp, mcrt_image.cpp), mcrt_group.cpp and the host half of mcrt_lbvh.hip share.  Nothing here launches, and only Staging waits.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <utility>
#include "../../include/mcrt.h"
#include "mcrt_internal.h"

// (an allocation the device cannot satisfy is MCRT_ERR_NOMEM, every other HIP failure MCRT_ERR_HIP)
#define HIP_TRY(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { (void)hipGetLastError(); return mcrt::set_error(e_ == hipErrorOutOfMemory ? MCRT_ERR_NOMEM : MCRT_ERR_HIP, "%s: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); } } while (0)
// a call that returns an mcrt_status and has set the message itself
#define MCRT_TRY(expr) do { const int rc_ = (expr); if (rc_) return rc_; } while (0)

// Owners, released in their destructors on the device that is current then (mcrt_destroy and mcrt_group_destroy make it the right one).
// A buffer holds `cap` elements.  alloc(n) replaces it by one of exactly n, grow(n) only when n exceeds the capacity; on failure it
// holds nothing.  Neither waits: whatever may still use the old buffer is waited for by the caller, who knows which wait that is.
template <class T, bool Pinned = false> struct Buf {
    T *p = nullptr; size_t cap = 0;
    Buf() = default;
    Buf(const Buf &) = delete; Buf &operator=(const Buf &) = delete;
    Buf(Buf &&o) noexcept { std::swap(p, o.p); std::swap(cap, o.cap); }
    Buf &operator=(Buf &&o) noexcept { std::swap(p, o.p); std::swap(cap, o.cap); return *this; }
    ~Buf() { reset(); }
    void reset() { if (p) { if (Pinned) hipHostFree(p); else hipFree(p); } p = nullptr; cap = 0; }
    hipError_t alloc(size_t n)
    {
        reset();
        if (n == 0) return hipSuccess;
        const hipError_t e = Pinned ? hipHostMalloc((void **)&p, sizeof(T) * n, hipHostMallocDefault) : hipMalloc((void **)&p, sizeof(T) * n);
        if (e != hipSuccess) p = nullptr; else cap = n;
        return e;
    }
    hipError_t grow(size_t n) { return n > cap ? alloc(n) : hipSuccess; }
    operator T *() const { return p; }
};
template <class T> using PinnedBuf = Buf<T, true>;
template <class H, hipError_t (*Destroy)(H)> struct Handle {   // an event or a stream: created by the caller into .h
    H h = nullptr;
    Handle() = default;
    Handle(const Handle &) = delete; Handle &operator=(const Handle &) = delete;
    Handle(Handle &&o) noexcept { std::swap(h, o.h); }
    Handle &operator=(Handle &&o) noexcept { std::swap(h, o.h); return *this; }
    ~Handle() { if (h) Destroy(h); }
    operator H() const { return h; }
};
using Event = Handle<hipEvent_t, hipEventDestroy>;
using Stream = Handle<hipStream_t, hipStreamDestroy>;

// an ORDERING event (no timing), made on first use
inline hipError_t ensure_event(Event &e) { return e.h ? hipSuccess : hipEventCreateWithFlags(&e.h, hipEventDisableTiming); }

// whether p is device memory; anything HIP does not know is the caller's host memory (and the lookup's error is cleared)
inline bool is_device_pointer(const void *p)
{
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, p) == hipSuccess && at.type == hipMemoryTypeDevice) return true;
    (void)hipGetLastError();
    return false;
}

// A host array of the caller's on the device by way of pinned memory its owner keeps, so that the caller's array is free the moment the
// call returns (the lifetime rule of include/mcrt.h).  begin(n) makes room for n floats -- the device buffer, the pinned buffer and the
// event together, all or none; a buffer that is replaced may still be read by what is queued on st, so st is waited for first, which a
// first allocation has no need of --, waits for the previous copy's event, whose source the pinned buffer still is, and hands out the
// pinned pointer.  The caller fills it; commit(n) enqueues the copy on st and records the event.  Nothing else waits for the device.
struct Staging {
    Buf<float> dev; PinnedBuf<float> pin; Event ev; bool pending = false;
    int begin(size_t n, hipStream_t st, float **out)
    {
        if (pending) { HIP_TRY(hipEventSynchronize(ev)); pending = false; }
        if (n > dev.cap) {
            if (dev) HIP_TRY(hipStreamSynchronize(st));
            Buf<float> d; PinnedBuf<float> h; Event e;
            HIP_TRY(d.alloc(n));
            HIP_TRY(h.alloc(n));
            HIP_TRY(ensure_event(e));
            dev = std::move(d); pin = std::move(h); ev = std::move(e);
        }
        *out = pin;
        return MCRT_OK;
    }
    int commit(size_t n, hipStream_t st)
    {
        HIP_TRY(hipMemcpyAsync(dev, pin, 4 * n, hipMemcpyHostToDevice, st));
        HIP_TRY(hipEventRecord(ev, st));
        pending = true;
        return MCRT_OK;
    }
};
