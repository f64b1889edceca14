// devmem.hpp — owners of what the library holds on the device: the context (context.hpp), the 64-bit field's path (gf61_kernels.hip), the shards of
// a sharded context (sharded.hip) and the state structs of decode_state.hpp, direct.hip, update.hip, gf61_update.hip, scrub.hip and gf61_decode.hip.  A struct's destructor
// is its whole teardown, and this file is the only one that allocates or frees device or pinned memory, events or streams.  Host code only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <utility>

#include "internal.hpp"

// HIP_TRY for a step that returns the library's own codes: on with FASTECC_OK, out of the function with anything else
#define RC_TRY(expr)                          \
    do {                                      \
        const int rc_ = (expr);               \
        if (rc_ != FASTECC_OK) return rc_;    \
    } while (0)

namespace fastecc {

struct DeviceMem {
    static hipError_t get(void** p, size_t bytes) { return hipMalloc(p, bytes); }
    static void put(void* p) { (void)hipFree(p); }
    static const char* call() { return "hipMalloc"; }
};
struct PinnedMem {
    static hipError_t get(void** p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
    static void put(void* p) { (void)hipHostFree(p); }
    static const char* call() { return "hipHostMalloc"; }
};

// Move-only owner of one block of `capacity()` elements; reads as the T* it replaces (kernel arguments, pointer arithmetic, null tests).
// alloc / grow return what HIP_TRY returns (hip_fail: the error detail is set, the HIP error cleared); the try_ forms leave both to the caller.
template <class T, class Mem = DeviceMem> class Buf {
public:
    Buf() = default;
    Buf(Buf&& o) noexcept { swap(o); }
    Buf& operator=(Buf&& o) noexcept
    {
        if (this != &o) {
            reset();
            swap(o);
        }
        return *this;
    }
    ~Buf() { reset(); }
    T* get() const { return p_; }
    operator T*() const { return p_; }
    uint64_t capacity() const { return cap_; }
    void reset()
    {
        if (p_) Mem::put(p_);
        p_ = nullptr;
        cap_ = 0;
    }
    void swap(Buf& o) noexcept
    {
        std::swap(p_, o.p_);
        std::swap(cap_, o.cap_);
    }
    // n elements unless the buffer holds some already (whatever their number)
    hipError_t try_alloc(uint64_t n)
    {
        if (p_) return hipSuccess;
        const hipError_t e = Mem::get((void**)&p_, n * sizeof(T));
        if (e != hipSuccess) p_ = nullptr;
        else cap_ = n;
        return e;
    }
    // grow-only: at least n elements, contents not kept; a failed allocation leaves nothing (the old block is gone as well)
    hipError_t try_grow(uint64_t n)
    {
        if (n <= cap_) return hipSuccess;
        reset();
        return try_alloc(n);
    }
    int alloc(uint64_t n) { return code(try_alloc(n)); }
    int grow(uint64_t n) { return code(try_grow(n)); }

private:
    static int code(hipError_t e) { return e == hipSuccess ? FASTECC_OK : hip_fail(e, Mem::call()); }
    T* p_ = nullptr;
    uint64_t cap_ = 0;
};
template <class T> using DeviceBuf = Buf<T, DeviceMem>;
template <class T> using PinnedBuf = Buf<T, PinnedMem>;

// An event created at its first use: without timing (Event), or one of a pair whose interval is read (TimedEvent: the profiler's records).
// create returns what HIP_TRY returns; try_create leaves the error and its detail to the caller.
template <unsigned Flags> class EventOf {
public:
    EventOf() = default;
    EventOf(EventOf&& o) noexcept { std::swap(ev_, o.ev_); }
    EventOf& operator=(EventOf&& o) noexcept
    {
        std::swap(ev_, o.ev_);  // (the other side destroys what this one held)
        return *this;
    }
    ~EventOf()
    {
        if (ev_) (void)hipEventDestroy(ev_);
    }
    hipError_t try_create() { return ev_ ? hipSuccess : hipEventCreateWithFlags(&ev_, Flags); }
    int create()
    {
        const hipError_t e = try_create();
        return e == hipSuccess ? FASTECC_OK : hip_fail(e, "hipEventCreateWithFlags");
    }
    operator hipEvent_t() const { return ev_; }

private:
    hipEvent_t ev_ = nullptr;
};
using Event = EventOf<hipEventDisableTiming>;
using TimedEvent = EventOf<hipEventDefault>;

// A non-blocking stream of the library's own, created at its first use.  The destructor does not wait: whoever must see the stream's work
// finished synchronises it first (fastecc_destroy does).
class Stream {
public:
    Stream() = default;
    Stream(const Stream&) = delete;
    Stream& operator=(const Stream&) = delete;
    ~Stream() { reset(); }
    void reset()
    {
        if (st_) (void)hipStreamDestroy(st_);
        st_ = nullptr;
    }
    hipError_t try_create() { return st_ ? hipSuccess : hipStreamCreateWithFlags(&st_, hipStreamNonBlocking); }
    int create()
    {
        const hipError_t e = try_create();
        return e == hipSuccess ? FASTECC_OK : hip_fail(e, "hipStreamCreateWithFlags");
    }
    operator hipStream_t() const { return st_; }

private:
    hipStream_t st_ = nullptr;
};

// One call's list, written on the host and read by kernels: the pinned buffer the call fills, its device copy (an internal buffer: ordered between
// streams by the context's buf_event) and the event of the copy between them, after which the pinned side may be written again.
template <class T> struct StagedList {
    PinnedBuf<T> host;
    DeviceBuf<T> dev;
    Event copied;
    bool pending = false;  // a copy out of `host` may still be under way

    // Room for `entries` entries, `host` free to be written: a call whose predecessor's list is still on its way to the device waits for that copy's
    // event (not for the device); growing calls wait_idle() — the host-side wait for the kernels that read `dev` — and then replaces both buffers.
    template <class WaitIdle> int reserve(uint64_t entries, WaitIdle wait_idle)
    {
        RC_TRY(copied.create());
        if (pending) {
            HIP_TRY(hipEventSynchronize(copied));
            pending = false;
        }
        if (entries <= dev.capacity()) return FASTECC_OK;
        const uint64_t cap = std::max<uint64_t>(std::max<uint64_t>(entries, 2 * dev.capacity()), 4096);
        RC_TRY(wait_idle());
        host.reset();
        dev.reset();
        RC_TRY(host.alloc(cap));
        return dev.alloc(cap);
    }
    // the first `entries` entries go to the device on `st`
    int publish(uint64_t entries, hipStream_t st)
    {
        HIP_TRY(hipMemcpyAsync(dev.get(), host.get(), entries * sizeof(T), hipMemcpyHostToDevice, st));
        HIP_TRY(hipEventRecord(copied, st));
        pending = true;
        return FASTECC_OK;
    }
};

// Internal contexts and passes: owned through the object's own destroy function; reads as the T* it replaces
template <class T, void (*Destroy)(T*)> class Owned {
public:
    Owned() = default;
    Owned(Owned&& o) noexcept { std::swap(p_, o.p_); }
    Owned& operator=(Owned&& o) noexcept
    {
        std::swap(p_, o.p_);  // (the other side destroys what this one held)
        return *this;
    }
    ~Owned() { reset(); }
    T* get() const { return p_; }
    operator T*() const { return p_; }
    T* operator->() const { return p_; }
    void reset(T* p = nullptr)
    {
        if (p_) Destroy(p_);
        p_ = p;
    }
    T** fill()  // for a create function's out parameter; holds nothing on entry
    {
        reset();
        return &p_;
    }

private:
    T* p_ = nullptr;
};
inline void destroy_ctx(fastecc_ctx* c) { (void)fastecc_destroy(c); }
using CtxPtr = Owned<fastecc_ctx, destroy_ctx>;
using DirectPassPtr = Owned<DirectPass, direct_pass_free>;
using PatternSetPtr = Owned<PatternSet, destroy_pattern_set>;

}  // namespace fastecc
