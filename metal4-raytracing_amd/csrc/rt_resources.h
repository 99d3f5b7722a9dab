// rt_resources.h — move-only owners of the four kinds of HIP resource the library holds: device
// buffer, pinned host block, stream, event.  Each releases in its destructor, so whatever owns one
// (rt_ctx, FrameSlot, Geo: rt_ctx.h) frees it by being destroyed, on every path.  Internal.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

namespace rt {

template <class H, hipError_t (*Release)(H)>
struct Owned {
    H h = nullptr;
    Owned() = default;
    Owned(Owned&& o) noexcept : h(o.h) { o.h = nullptr; }
    Owned& operator=(Owned&& o) noexcept {
        if (this != &o) {
            reset();
            h = o.h;
            o.h = nullptr;
        }
        return *this;
    }
    ~Owned() { reset(); }
    void reset() {
        if (h) (void)Release(h);
        h = nullptr;
    }
    operator H() const { return h; }
};

struct Stream : Owned<hipStream_t, hipStreamDestroy> {
    hipError_t create() {
        reset();
        return hipStreamCreateWithFlags(&h, hipStreamNonBlocking);
    }
};

struct Event : Owned<hipEvent_t, hipEventDestroy> {
    hipError_t create(unsigned flags = hipEventDefault) {
        reset();
        return hipEventCreateWithFlags(&h, flags);
    }
};

// Pinned host memory, typed by what the block holds.
template <class T>
struct Pinned : Owned<void*, hipHostFree> {
    hipError_t alloc(size_t bytes) {
        reset();
        return hipHostMalloc(&h, bytes, 0);
    }
    T* get() const { return (T*)h; }
};

// Device memory.  reserve / release are the only code that allocates or frees it, and both keep
// the caller's running tally of bytes held (rt_stats.device_bytes), so no buffer can be left out
// of the count.  (The destructor leaves the tally alone: it runs when the tally's owner dies.)
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr, o.bytes = 0; }
    DevBuf& operator=(DevBuf&&) = delete;   // a live buffer leaves only through release (the tally)
    ~DevBuf() {
        if (p) (void)hipFree(p);
    }
    // Room for `n` bytes: kept as it is when large enough, freed and allocated anew otherwise;
    // n == 0 frees.
    hipError_t reserve(size_t n, size_t& tally) {
        if (p && bytes >= n && n > 0) return hipSuccess;
        release(tally);
        if (n == 0) return hipSuccess;
        hipError_t e = hipMalloc(&p, n);
        if (e != hipSuccess) {
            p = nullptr;
            return e;
        }
        bytes = n;
        tally += n;
        return hipSuccess;
    }
    void release(size_t& tally) {
        if (p) (void)hipFree(p);
        tally -= bytes;
        p = nullptr;
        bytes = 0;
    }
};

}  // namespace rt
