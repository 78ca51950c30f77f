// libmod16hip.so, host side: the owners of what the HIP runtime hands out. Every handle struct
// (mod16_ctx, mod16_graph, mod16_batch, mod16_mcmc, mod16_ensemble) holds its device and page-locked
// memory, streams, events and graphs through these; a raw pointer in one of them is a view. All are
// move-only and release in their destructor, so a half-built object and a failure path free what they
// made by going out of scope.
#pragma once
#include <hip/hip_runtime.h>

#include <utility>

#include "../../../include/mod16_hip.h"

struct mod16_ctx;
static int fail(mod16_ctx* ctx, int code, const char* msg);     // (internal.hpp)

struct DevApi {
    static hipError_t alloc(void** p, size_t bytes) { return hipMalloc(p, bytes); }
    static void free(void* p) { (void)hipFree(p); }
};
struct PinnedApi {
    static hipError_t alloc(void** p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
    static void free(void* p) { (void)hipHostFree(p); }
};
// One block of device (DevMem) or page-locked (PinnedMem) memory and its size.
template <typename Api> class Owned {
    void* p_ = nullptr;
    size_t bytes_ = 0;
public:
    Owned() = default;
    Owned(Owned&& o) noexcept : p_(std::exchange(o.p_, nullptr)), bytes_(std::exchange(o.bytes_, 0)) {}
    Owned& operator=(Owned&& o) noexcept {
        if (this != &o) { release(); p_ = std::exchange(o.p_, nullptr); bytes_ = std::exchange(o.bytes_, 0); }
        return *this;
    }
    ~Owned() { release(); }
    void* get() const { return p_; }
    template <typename T> T* as() const { return static_cast<T*>(p_); }
    size_t bytes() const { return bytes_; }
    explicit operator bool() const { return p_ != nullptr; }
    void release() {
        if (p_) Api::free(p_);
        p_ = nullptr;
        bytes_ = 0;
    }
    // Memory that cannot be had is MOD16_ERR_NOMEM with `what` as the message, not a HIP error: the
    // owner is empty and the runtime's last error is cleared, so that the next hipGetLastError() behind
    // a launch on this thread reports its own launch.
    int alloc(mod16_ctx* ctx, size_t bytes, const char* what) {
        release();
        if (Api::alloc(&p_, bytes) != hipSuccess) {
            (void)hipGetLastError();
            p_ = nullptr;
            return fail(ctx, MOD16_ERR_NOMEM, what);
        }
        bytes_ = bytes;
        return MOD16_OK;
    }
    // room for `bytes`: the block only grows (a caller whose graphs or stream still use the old block
    // drops or synchronizes them first)
    int reserve(mod16_ctx* ctx, size_t bytes, const char* what) { return bytes_ >= bytes ? MOD16_OK : alloc(ctx, bytes, what); }
};
using DevMem = Owned<DevApi>;
using PinnedMem = Owned<PinnedApi>;

// A stream-ordered temporary of one call (hipMallocAsync): given back on its stream when the scope ends.
struct AsyncMem {
    void* p = nullptr;
    hipStream_t st;
    explicit AsyncMem(hipStream_t s) : st(s) {}
    AsyncMem(const AsyncMem&) = delete;
    AsyncMem& operator=(const AsyncMem&) = delete;
    ~AsyncMem() { release(); }
    void release() { if (p) (void)hipFreeAsync(std::exchange(p, nullptr), st); }
    int alloc(mod16_ctx* ctx, size_t bytes, const char* what) {
        if (hipMallocAsync(&p, bytes, st) == hipSuccess) return MOD16_OK;
        (void)hipGetLastError();
        p = nullptr;
        return fail(ctx, MOD16_ERR_NOMEM, what);
    }
};

struct Stream {
    hipStream_t s = nullptr;
    Stream() = default;
    Stream(const Stream&) = delete;
    Stream& operator=(const Stream&) = delete;
    ~Stream() { if (s) (void)hipStreamDestroy(s); }
    operator hipStream_t() const { return s; }
    // a non-blocking stream, made on first use
    hipError_t ensure() { return s ? hipSuccess : hipStreamCreateWithFlags(&s, hipStreamNonBlocking); }
};
struct Event {
    hipEvent_t e = nullptr;
    Event() = default;
    Event(const Event&) = delete;
    Event& operator=(const Event&) = delete;
    ~Event() { if (e) (void)hipEventDestroy(e); }
    operator hipEvent_t() const { return e; }
    hipError_t ensure(unsigned flags = hipEventDefault) { return e ? hipSuccess : hipEventCreateWithFlags(&e, flags); }
};
// GPU time of what is enqueued on a stream between start() and stop_ms()
struct EventTimer {
    Event e0, e1;
    hipError_t start(hipStream_t st) {
        hipError_t e = e0.ensure();
        if (e == hipSuccess) e = e1.ensure();
        return e == hipSuccess ? hipEventRecord(e0, st) : e;
    }
    // waits for the stream to reach this point
    int stop_ms(hipStream_t st, float* ms) {
        const bool ok = hipEventRecord(e1, st) == hipSuccess && hipEventSynchronize(e1) == hipSuccess &&
                        hipEventElapsedTime(ms, e0, e1) == hipSuccess;
        return ok ? MOD16_OK : MOD16_ERR_HIP;
    }
};
