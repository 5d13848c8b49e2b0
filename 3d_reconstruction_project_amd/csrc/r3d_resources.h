// Owning types for the GPU resources the host code holds: device buffers, pinned host buffers, events and streams.  Each is
// move-only and frees what it holds in its destructor, so a struct that has them as members needs no free list.  This header is
// the only place in csrc/ that calls the HIP create / free / destroy functions; every such call goes through the counted
// functions below, which keep the process-wide totals that r3d_debug_resources reports.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <atomic>
#include <utility>

#include "../../include/r3d.h"

int r3d_fail(r3d_ctx *ctx, int code, const char *fmt, ...);

// ---- live counts -------------------------------------------------------------------------------------------------------------------
struct r3d_live_counts {
    std::atomic<int64_t> device_allocs{0}, device_bytes{0}, pinned_allocs{0}, events{0}, streams{0};
};
inline r3d_live_counts r3d_live;

// owned_bytes: the size of a buffer an r3d_buf owns; 0 for a raw handle given to the caller (r3d_dev_alloc), whose size is unknown
// when it comes back
inline hipError_t r3d_hip_malloc(void **p, size_t bytes, size_t owned_bytes) {
    const hipError_t e = hipMalloc(p, bytes);
    if (e == hipSuccess) { r3d_live.device_allocs++; r3d_live.device_bytes += (int64_t)owned_bytes; }
    return e;
}
inline hipError_t r3d_hip_free(void *p, size_t owned_bytes) {
    const hipError_t e = hipFree(p);
    if (e == hipSuccess && p) { r3d_live.device_allocs--; r3d_live.device_bytes -= (int64_t)owned_bytes; }
    return e;
}
inline hipError_t r3d_hip_event_create(hipEvent_t *ev, unsigned flags = hipEventDefault) {
    const hipError_t e = flags == hipEventDefault ? hipEventCreate(ev) : hipEventCreateWithFlags(ev, flags);
    if (e == hipSuccess) r3d_live.events++;
    return e;
}
inline hipError_t r3d_hip_event_destroy(hipEvent_t ev) {
    const hipError_t e = hipEventDestroy(ev);
    if (e == hipSuccess) r3d_live.events--;
    return e;
}

// ---- device buffer -----------------------------------------------------------------------------------------------------------------
// how a buffer grows (r3d_buf::reserve)
struct r3d_grow {
    unsigned pad_div;        // the request is padded by bytes / pad_div + 4096; 0: the exact size
    bool alloc_first;        // true: allocate, copy, synchronise, free (contents can be kept; old and new exist together);
                             // false: synchronise, free, allocate (a multi-GiB volume never exists twice; nothing is kept)
    bool device_sync;        // the synchronisation before the old buffer goes: the whole device (lanes run on their own streams) or the stream
    const char *who;         // prefix of the allocation failure message
    const char *copy_failed; // message when the copy, the zeroing or their synchronisation fails (alloc_first only)
};
constexpr r3d_grow R3D_GROW_WORKSPACE = {8, false, true, "", ""};                                 // context workspaces (r3d_reserve)
constexpr r3d_grow R3D_GROW_MODEL = {2, true, false, "", "model grow copy failed"};               // resident model rows
constexpr r3d_grow R3D_GROW_VOXEL_TABLE = {2, false, false, "", ""};                              // resident model voxel table
constexpr r3d_grow R3D_GROW_TSDF = {0, true, false, "tsdf: ", "tsdf: growing a plane failed"};    // TSDF planes and tables

struct r3d_buf {
    void *p = nullptr;
    size_t cap = 0;

    r3d_buf() = default;
    r3d_buf(const r3d_buf &) = delete;
    r3d_buf &operator=(const r3d_buf &) = delete;
    r3d_buf(r3d_buf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    r3d_buf &operator=(r3d_buf &&o) noexcept {
        if (this != &o) {
            release();
            p = o.p; cap = o.cap;
            o.p = nullptr; o.cap = 0;
        }
        return *this;
    }
    ~r3d_buf() { release(); }

    void release() {
        if (p) (void)r3d_hip_free(p, cap);
        p = nullptr;
        cap = 0;
    }
    // exactly `bytes`, replacing whatever was held; no synchronisation and no message
    hipError_t alloc(size_t bytes) {
        release();
        const hipError_t e = r3d_hip_malloc(&p, bytes, bytes);
        if (e != hipSuccess) p = nullptr;
        else cap = bytes;
        return e;
    }
    // grow-only: at least `bytes`, by policy g.  alloc_first policies copy the first `keep` bytes of the old buffer, zero the rest
    // of the new one when zero_tail, and leave the old buffer in place when anything fails; the others leave the buffer empty.
    int reserve(r3d_ctx *ctx, hipStream_t st, size_t bytes, const r3d_grow &g, size_t keep = 0, bool zero_tail = false) {
        if (bytes <= cap) return R3D_OK;
        const size_t want = g.pad_div ? bytes + bytes / g.pad_div + 4096 : bytes;
        if (!g.alloc_first && p) {
            (void)(g.device_sync ? hipDeviceSynchronize() : hipStreamSynchronize(st));
            release();
        }
        r3d_buf nb;
        hipError_t e = nb.alloc(want);
        if (e != hipSuccess) return r3d_fail(ctx, R3D_E_OOM, "%shipMalloc(%zu) failed: %s", g.who, want, hipGetErrorString(e));
        if (p && keep) e = hipMemcpyAsync(nb.p, p, keep, hipMemcpyDeviceToDevice, st);
        if (e == hipSuccess && zero_tail) e = hipMemsetAsync((char *)nb.p + keep, 0, want - keep, st);
        if (e == hipSuccess && (p || zero_tail)) e = g.device_sync ? hipDeviceSynchronize() : hipStreamSynchronize(st);
        if (e != hipSuccess) return r3d_fail(ctx, R3D_E_HIP, "%s: %s", g.copy_failed, hipGetErrorString(e));
        *this = std::move(nb);
        return R3D_OK;
    }
};

// ---- pinned host buffer ------------------------------------------------------------------------------------------------------------
struct r3d_pinned {
    void *p = nullptr;

    r3d_pinned() = default;
    r3d_pinned(const r3d_pinned &) = delete;
    r3d_pinned &operator=(const r3d_pinned &) = delete;
    r3d_pinned(r3d_pinned &&o) noexcept : p(o.p) { o.p = nullptr; }
    r3d_pinned &operator=(r3d_pinned &&o) noexcept {
        if (this != &o) { release(); p = o.p; o.p = nullptr; }
        return *this;
    }
    ~r3d_pinned() { release(); }

    void release() {
        if (p && hipHostFree(p) == hipSuccess) r3d_live.pinned_allocs--;
        p = nullptr;
    }
    hipError_t alloc(size_t bytes, unsigned flags) {
        release();
        const hipError_t e = hipHostMalloc(&p, bytes, flags);
        if (e != hipSuccess) p = nullptr;
        else r3d_live.pinned_allocs++;
        return e;
    }
};

// ---- events ------------------------------------------------------------------------------------------------------------------------
// N events, created one by one or all at once; a raw hipEvent_t array to the code that records and reads them
template <int N> struct r3d_events {
    hipEvent_t e[N] = {};

    r3d_events() = default;
    r3d_events(const r3d_events &) = delete;
    r3d_events &operator=(const r3d_events &) = delete;
    r3d_events(r3d_events &&o) noexcept { for (int i = 0; i < N; i++) { e[i] = o.e[i]; o.e[i] = nullptr; } }
    r3d_events &operator=(r3d_events &&o) noexcept {
        if (this != &o) { release(); for (int i = 0; i < N; i++) { e[i] = o.e[i]; o.e[i] = nullptr; } }
        return *this;
    }
    ~r3d_events() { release(); }

    void release() {
        for (auto &x : e) {
            if (x) (void)r3d_hip_event_destroy(x);
            x = nullptr;
        }
    }
    hipError_t create(int i, unsigned flags = hipEventDefault) {
        const hipError_t err = r3d_hip_event_create(&e[i], flags);
        if (err != hipSuccess) e[i] = nullptr;
        return err;
    }
    hipError_t create_all(unsigned flags = hipEventDefault) {   // stops at the first failure; the destructor takes what exists
        for (int i = 0; i < N; i++)
            if (!e[i])
                if (const hipError_t err = create(i, flags)) return err;
        return hipSuccess;
    }
    hipEvent_t operator[](int i) const { return e[i]; }
};
struct r3d_event : r3d_events<1> {
    hipError_t create(unsigned flags = hipEventDefault) { return r3d_events<1>::create(0, flags); }
    operator hipEvent_t() const { return e[0]; }
};

// ---- stream ------------------------------------------------------------------------------------------------------------------------
struct r3d_stream {
    hipStream_t s = nullptr;

    r3d_stream() = default;
    r3d_stream(const r3d_stream &) = delete;
    r3d_stream &operator=(const r3d_stream &) = delete;
    r3d_stream(r3d_stream &&o) noexcept : s(o.s) { o.s = nullptr; }
    r3d_stream &operator=(r3d_stream &&o) noexcept {
        if (this != &o) { release(); s = o.s; o.s = nullptr; }
        return *this;
    }
    ~r3d_stream() { release(); }

    void release() {
        if (s && hipStreamDestroy(s) == hipSuccess) r3d_live.streams--;
        s = nullptr;
    }
    hipError_t create(unsigned flags) {
        release();
        const hipError_t e = hipStreamCreateWithFlags(&s, flags);
        if (e != hipSuccess) s = nullptr;
        else r3d_live.streams++;
        return e;
    }
    operator hipStream_t() const { return s; }
};
