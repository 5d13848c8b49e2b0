// api.hip -- context, memory/timing helpers and the  extern "C" entry points declared in include/r3d.h.
#include <dlfcn.h>
#include <mutex>
#include <stdarg.h>
#include <stdlib.h>
#include <string.h>

#include "r3d_internal.h"

static std::string g_init_err;

// ---- roctx markers, resolved lazily with dlopen (no link-time dependency on a profiler library) -------------------------------
namespace {
typedef int (*roctx_push_fn)(const char *);
typedef int (*roctx_pop_fn)();
roctx_push_fn g_roctx_push = nullptr;
roctx_pop_fn g_roctx_pop = nullptr;
std::once_flag g_roctx_once;   // one ctx per calling thread is the documented model: the lookup must be safe under concurrent first calls
void roctx_lookup() {
    const char *e = getenv("R3D_ROCTX");
    if (e && !strcmp(e, "0")) return;
    for (const char *lib : {"librocprofiler-sdk-roctx.so.1", "librocprofiler-sdk-roctx.so", "libroctx64.so.4", "libroctx64.so"}) {
        void *h = dlopen(lib, RTLD_NOW | RTLD_GLOBAL);
        if (!h) continue;
        roctx_push_fn pu = (roctx_push_fn)dlsym(h, "roctxRangePushA");
        roctx_pop_fn po = (roctx_pop_fn)dlsym(h, "roctxRangePop");
        if (pu && po) { g_roctx_pop = po; g_roctx_push = pu; return; }
    }
}
}  // namespace
bool r3d_roctx_push(const char *name) {
    std::call_once(g_roctx_once, roctx_lookup);   // both pointers are published before call_once returns on any thread
    if (!g_roctx_push) return false;
    (void)g_roctx_push(name);
    return true;
}
void r3d_roctx_pop() {
    if (g_roctx_pop) (void)g_roctx_pop();
}


int r3d_fail(r3d_ctx *ctx, int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (ctx) ctx->err = buf;
    else g_init_err = buf;
    return code;
}

void r3d_prof_harvest(r3d_ctx *ctx, r3d_prof_set &ps) {
    ps.pending = false;
    if (ps.n == 0 || hipEventSynchronize(ps.ev[ps.n]) != hipSuccess) return;
    for (int i = 0; i < ps.n; i++) {
        float t = 0;
        if (hipEventElapsedTime(&t, ps.ev[i], ps.ev[i + 1]) != hipSuccess) continue;
        int k = 0;
        while (k < ctx->n_acc && strcmp(ctx->acc_name[k], ps.name[i]) != 0) k++;
        if (k == ctx->n_acc) {
            if (ctx->n_acc >= R3D_MAX_PROF) continue;
            ctx->acc_name[k] = ps.name[i];
            ctx->acc_ms[k] = 0;
            ctx->acc_cnt[k] = 0;
            ctx->n_acc++;
        }
        ctx->acc_ms[k] += t;
        ctx->acc_cnt[k]++;
    }
}

extern "C" {

int r3d_init(int device, r3d_ctx **out) {
    if (!out) return r3d_fail(nullptr, R3D_E_BADARG, "r3d_init: out is NULL");
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return r3d_fail(nullptr, R3D_E_NODEVICE, "r3d_init: no HIP device (%s)", e != hipSuccess ? hipGetErrorString(e) : "count=0");
    if (device < 0 || device >= n) return r3d_fail(nullptr, R3D_E_BADARG, "r3d_init: device %d out of range [0,%d)", device, n);
    hipDeviceProp_t prop;
    if ((e = hipGetDeviceProperties(&prop, device)) != hipSuccess)
        return r3d_fail(nullptr, R3D_E_HIP, "hipGetDeviceProperties: %s", hipGetErrorString(e));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return r3d_fail(nullptr, R3D_E_NODEVICE, "r3d_init: device %d is %s; this library contains gfx950 code only", device, prop.gcnArchName);
    r3d_ctx *ctx = new (std::nothrow) r3d_ctx();
    if (!ctx) return r3d_fail(nullptr, R3D_E_OOM, "r3d_init: out of host memory");
    ctx->device = device;
    if ((e = hipSetDevice(device)) != hipSuccess || (e = ctx->own_stream.create(hipStreamNonBlocking)) != hipSuccess) {
        int rc = r3d_fail(nullptr, R3D_E_HIP, "r3d_init: %s", hipGetErrorString(e));
        delete ctx;
        return rc;
    }
    ctx->stream = ctx->own_stream;
    *out = ctx;
    return R3D_OK;
}

void r3d_destroy(r3d_ctx *ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    (void)hipDeviceSynchronize();
    delete ctx;   // every buffer, pinned block, event and stream is a member that frees itself (r3d_resources.h)
}

int r3d_debug_resources(r3d_resource_counts *out) {
    if (!out) return R3D_E_BADARG;
    out->device_allocs = r3d_live.device_allocs.load();
    out->device_bytes = r3d_live.device_bytes.load();
    out->pinned_allocs = r3d_live.pinned_allocs.load();
    out->events = r3d_live.events.load();
    out->streams = r3d_live.streams.load();
    return R3D_OK;
}

const char *r3d_last_error(const r3d_ctx *ctx) { return ctx ? ctx->err.c_str() : g_init_err.c_str(); }

int r3d_sync(r3d_ctx *ctx) {
    R3D_ROCTX_RANGE("r3d_sync");
    if (!ctx) return R3D_E_BADARG;
    R3D_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return R3D_OK;
}

int r3d_set_stream(r3d_ctx *ctx, void *s) {
    if (!ctx) return R3D_E_BADARG;
    ctx->stream = s ? (hipStream_t)s : ctx->own_stream;
    return R3D_OK;
}
void *r3d_get_stream(r3d_ctx *ctx) { return ctx ? (void *)ctx->stream : nullptr; }
int r3d_stream_wait_event(r3d_ctx *ctx, void *ev) {
    if (!ctx || !ev) return R3D_E_BADARG;
    R3D_HIP(ctx, hipSetDevice(ctx->device));
    R3D_HIP(ctx, hipStreamWaitEvent(ctx->stream, (hipEvent_t)ev, 0));
    return R3D_OK;
}

int r3d_debug_streambench(r3d_ctx *ctx, int32_t mode, int32_t rows, uint64_t row_bytes, int32_t write, int32_t delay, int32_t reps, float *ms) {
    R3D_ROCTX_RANGE("r3d_debug_streambench");
    if (!ctx || !ms || rows <= 0 || reps <= 0) return R3D_E_BADARG;
    return r3d_streambench_run(ctx, mode, rows, row_bytes, write, delay, reps, ms);
}

int r3d_selftest(r3d_ctx *ctx) {
    R3D_ROCTX_RANGE("r3d_selftest");
    if (!ctx) return R3D_E_BADARG;
    return r3d_selftest_run(ctx);
}

int r3d_dev_alloc(r3d_ctx *ctx, uint64_t bytes, void **out) {
    R3D_ROCTX_RANGE("r3d_dev_alloc");
    if (!ctx || !out) return R3D_E_BADARG;
    R3D_HIP(ctx, hipSetDevice(ctx->device));
    hipError_t e = r3d_hip_malloc(out, bytes ? bytes : 1, 0);
    if (e != hipSuccess) return r3d_fail(ctx, R3D_E_OOM, "hipMalloc(%llu): %s", (unsigned long long)bytes, hipGetErrorString(e));
    return R3D_OK;
}
int r3d_dev_free(r3d_ctx *ctx, void *p) {
    R3D_ROCTX_RANGE("r3d_dev_free");
    if (!ctx) return R3D_E_BADARG;
    R3D_HIP(ctx, hipStreamSynchronize(ctx->stream));
    R3D_HIP(ctx, r3d_hip_free(p, 0));
    return R3D_OK;
}
int r3d_copy_h2d(r3d_ctx *ctx, void *d, const void *h, uint64_t bytes) {
    R3D_ROCTX_RANGE("r3d_copy_h2d");
    if (!ctx || (!d && bytes) || (!h && bytes)) return R3D_E_BADARG;
    R3D_HIP(ctx, hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, ctx->stream));
    R3D_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return R3D_OK;
}
int r3d_copy_d2h(r3d_ctx *ctx, void *h, const void *d, uint64_t bytes) {
    R3D_ROCTX_RANGE("r3d_copy_d2h");
    if (!ctx || (!d && bytes) || (!h && bytes)) return R3D_E_BADARG;
    R3D_HIP(ctx, hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, ctx->stream));
    R3D_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return R3D_OK;
}
int r3d_event_create(r3d_ctx *ctx, void **out) {
    if (!ctx || !out) return R3D_E_BADARG;
    hipEvent_t e;
    R3D_HIP(ctx, r3d_hip_event_create(&e));
    *out = (void *)e;
    return R3D_OK;
}
int r3d_event_destroy(r3d_ctx *ctx, void *e) {
    if (!ctx) return R3D_E_BADARG;
    R3D_HIP(ctx, r3d_hip_event_destroy((hipEvent_t)e));
    return R3D_OK;
}
int r3d_event_record(r3d_ctx *ctx, void *e) {
    if (!ctx || !e) return R3D_E_BADARG;
    R3D_HIP(ctx, hipEventRecord((hipEvent_t)e, ctx->stream));
    return R3D_OK;
}
int r3d_event_elapsed_ms(r3d_ctx *ctx, void *a, void *b, float *ms) {
    if (!ctx || !a || !b || !ms) return R3D_E_BADARG;
    R3D_HIP(ctx, hipEventSynchronize((hipEvent_t)b));
    R3D_HIP(ctx, hipEventElapsedTime(ms, (hipEvent_t)a, (hipEvent_t)b));
    return R3D_OK;
}

int r3d_set_profiling(r3d_ctx *ctx, int enabled) {
    if (!ctx) return R3D_E_BADARG;
    ctx->profiling = enabled != 0;
    return R3D_OK;
}

int r3d_sgbm_profile(r3d_ctx *ctx, float *ms, int32_t max_slots, char *names, int32_t names_bytes) {
    if (!ctx) return R3D_E_BADARG;
    for (r3d_sgm_ws &ws : ctx->ws)
        for (auto &ps : ws.prof)
            if (ps.pending) r3d_prof_harvest(ctx, ps);
    int n = ctx->n_acc < max_slots ? ctx->n_acc : max_slots;
    size_t off = 0;
    for (int i = 0; i < n; i++) {
        if (ms) ms[i] = ctx->acc_cnt[i] ? (float)(ctx->acc_ms[i] / ctx->acc_cnt[i]) : 0.f;
        if (names) {
            size_t len = strlen(ctx->acc_name[i]) + 1;
            if (off + len <= (size_t)names_bytes) { memcpy(names + off, ctx->acc_name[i], len); off += len; }
        }
    }
    ctx->n_acc = 0;
    return n;
}

// The entry points without _cn are the single-channel case of the ones with it.
int r3d_sgbm_compute_dev(r3d_ctx *ctx, const r3d_sgbm_params *p, const uint8_t *d_left, const uint8_t *d_right, int32_t w,
                         int32_t h, int32_t stride, int16_t *d_disp) {
    R3D_ROCTX_RANGE("r3d_sgbm_compute_dev");
    if (!ctx) return R3D_E_BADARG;
    return r3d_sgm_run(ctx, 0, ctx->stream, p, d_left, d_right, w, h, stride, 1, d_disp);
}

int r3d_sgbm_compute_cn_dev(r3d_ctx *ctx, const r3d_sgbm_params *p, const uint8_t *d_left, const uint8_t *d_right, int32_t w,
                            int32_t h, int32_t stride, int32_t cn, int16_t *d_disp) {
    R3D_ROCTX_RANGE("r3d_sgbm_compute_cn_dev");
    if (!ctx) return R3D_E_BADARG;
    return r3d_sgm_run(ctx, 0, ctx->stream, p, d_left, d_right, w, h, stride, cn, d_disp);
}

int r3d_sgbm_compute_batch_dev(r3d_ctx *ctx, const r3d_sgbm_params *p, int32_t n, const uint8_t *const *d_left,
                               const uint8_t *const *d_right, int32_t w, int32_t h, int32_t stride, int16_t *const *d_disp) {
    return r3d_sgbm_compute_batch_cn_dev(ctx, p, n, d_left, d_right, w, h, stride, 1, d_disp, nullptr);
}

int r3d_sgbm_compute_batch_events_dev(r3d_ctx *ctx, const r3d_sgbm_params *p, int32_t n, const uint8_t *const *d_left,
                                      const uint8_t *const *d_right, int32_t w, int32_t h, int32_t stride, int16_t *const *d_disp,
                                      void *const *done_events) {
    return r3d_sgbm_compute_batch_cn_dev(ctx, p, n, d_left, d_right, w, h, stride, 1, d_disp, done_events);
}

int r3d_sgbm_compute_batch_cn_dev(r3d_ctx *ctx, const r3d_sgbm_params *p, int32_t n, const uint8_t *const *d_left,
                                  const uint8_t *const *d_right, int32_t w, int32_t h, int32_t stride, int32_t cn, int16_t *const *d_disp,
                                  void *const *done_events) {
    R3D_ROCTX_RANGE("r3d_sgbm_compute_batch_dev");
    if (!ctx) return R3D_E_BADARG;
    if (cn != 1 && cn != 3) return r3d_fail(ctx, R3D_E_BADARG, "sgbm batch: images must have 1 or 3 channels, got %d", cn);
    if (n < 0 || (n > 0 && (!d_left || !d_right || !d_disp))) return r3d_fail(ctx, R3D_E_BADARG, "sgbm batch: bad argument");
    if (n == 0) return R3D_OK;
    R3D_HIP(ctx, hipSetDevice(ctx->device));
    // maps in flight: R3D_SGM_LANES (default 3; measured A/B values 2 .. 6)
    static const int max_lanes = [] { const char *e = getenv("R3D_SGM_LANES"); const int v = e ? atoi(e) : R3D_SGM_LANES; return v < 1 ? 1 : (v > R3D_SGM_MAX_LANES ? R3D_SGM_MAX_LANES : v); }();
    const int lanes = n < max_lanes ? n : max_lanes;
    if (!ctx->fork_ev) R3D_HIP(ctx, ctx->fork_ev.create(hipEventDisableTiming));
    for (int l = 0; l < lanes; l++) {
        r3d_sgm_ws &ws = ctx->ws[l];
        if (!ws.stream) R3D_HIP(ctx, ws.stream.create(hipStreamNonBlocking));
        if (!ws.done) R3D_HIP(ctx, ws.done.create(hipEventDisableTiming));
    }
    // fork: every lane starts after whatever is already queued on the context stream
    R3D_HIP(ctx, hipEventRecord(ctx->fork_ev, ctx->stream));
    for (int l = 0; l < lanes; l++) R3D_HIP(ctx, hipStreamWaitEvent(ctx->ws[l].stream, ctx->fork_ev, 0));
    int rc = R3D_OK;
    for (int i = 0; i < n && rc == R3D_OK; i++) {
        const int l = i % lanes;
        rc = r3d_sgm_run(ctx, l, ctx->ws[l].stream, p, d_left[i], d_right[i], w, h, stride, cn, d_disp[i]);
        if (rc == R3D_OK && done_events && done_events[i]) {
            // a stale or foreign-device event handle fails here: remember it, stop launching, and STILL run the join below
            const hipError_t e = hipEventRecord((hipEvent_t)done_events[i], ctx->ws[l].stream);
            if (e != hipSuccess) rc = r3d_fail(ctx, R3D_E_HIP, "sgbm batch: recording done_events[%d] failed: %s", i, hipGetErrorString(e));
        }
    }
    // join: the context stream continues after every lane has drained -- on EVERY exit path after the fork, so that maps already
    // enqueued on the lanes stay ordered before whatever the caller queues next on the context stream
    for (int l = 0; l < lanes; l++) {
        hipError_t e = hipEventRecord(ctx->ws[l].done, ctx->ws[l].stream);
        if (e == hipSuccess) e = hipStreamWaitEvent(ctx->stream, ctx->ws[l].done, 0);
        if (e != hipSuccess) {                 // cannot order the lane by an event: drain it on the host instead
            (void)hipStreamSynchronize(ctx->ws[l].stream);
            if (rc == R3D_OK) rc = r3d_fail(ctx, R3D_E_HIP, "sgbm batch: joining lane %d failed: %s", l, hipGetErrorString(e));
        }
    }
    return rc;
}

int r3d_sgbm_compute(r3d_ctx *ctx, const r3d_sgbm_params *p, const uint8_t *left, const uint8_t *right, int32_t w, int32_t h,
                     int32_t stride, int16_t *disp) {
    return r3d_sgbm_compute_cn(ctx, p, left, right, w, h, stride, 1, disp);
}

int r3d_sgbm_compute_cn(r3d_ctx *ctx, const r3d_sgbm_params *p, const uint8_t *left, const uint8_t *right, int32_t w, int32_t h,
                        int32_t stride, int32_t cn, int16_t *disp) {
    R3D_ROCTX_RANGE("r3d_sgbm_compute");
    if (!ctx) return R3D_E_BADARG;
    if (!left || !right || !disp) return r3d_fail(ctx, R3D_E_BADARG, "sgbm: null host pointer");
    if (cn != 1 && cn != 3) return r3d_fail(ctx, R3D_E_BADARG, "sgbm: images must have 1 or 3 channels, got %d", cn);
    if (w <= 0 || h <= 0 || stride < w * cn) return r3d_fail(ctx, R3D_E_BADARG, "sgbm: bad size %dx%d (%d channel(s)) stride %d", w, h, cn, stride);
    R3D_HIP(ctx, hipSetDevice(ctx->device));
    const size_t ib = (size_t)stride * h, ob = (size_t)w * h * 2;
    int rc;
    if ((rc = r3d_reserve(ctx, ctx->img_l, ib)) || (rc = r3d_reserve(ctx, ctx->img_r, ib)) || (rc = r3d_reserve(ctx, ctx->out, ob))) return rc;
    R3D_HIP(ctx, hipMemcpyAsync(ctx->img_l.p, left, ib, hipMemcpyHostToDevice, ctx->stream));
    R3D_HIP(ctx, hipMemcpyAsync(ctx->img_r.p, right, ib, hipMemcpyHostToDevice, ctx->stream));
    if ((rc = r3d_sgm_run(ctx, 0, ctx->stream, p, (const uint8_t *)ctx->img_l.p, (const uint8_t *)ctx->img_r.p, w, h, stride, cn, (int16_t *)ctx->out.p))) return rc;
    if ((rc = r3d_download(ctx, disp, (const int16_t *)ctx->out.p, (size_t)w * h))) return rc;
    R3D_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return R3D_OK;
}

int r3d_filter_speckles(r3d_ctx *ctx, int16_t *img, int32_t w, int32_t h, int32_t new_val, int32_t max_speckle_size, int32_t max_diff) {
    R3D_ROCTX_RANGE("r3d_filter_speckles");
    if (!ctx) return R3D_E_BADARG;
    if (!img || w <= 0 || h <= 0) return r3d_fail(ctx, R3D_E_BADARG, "filter_speckles: bad argument");
    R3D_HIP(ctx, hipSetDevice(ctx->device));
    const size_t bytes = (size_t)w * h * 2;
    int rc;
    if ((rc = r3d_reserve(ctx, ctx->out, bytes))) return rc;
    R3D_HIP(ctx, hipMemcpyAsync(ctx->out.p, img, bytes, hipMemcpyHostToDevice, ctx->stream));
    if ((rc = r3d_speckle_run(ctx, ctx->ws[0], ctx->stream, (int16_t *)ctx->out.p, w, h, new_val, max_speckle_size, max_diff))) return rc;
    if ((rc = r3d_download(ctx, img, (const int16_t *)ctx->out.p, (size_t)w * h))) return rc;
    R3D_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return R3D_OK;
}

int r3d_sgbm_debug_fetch(r3d_ctx *ctx, int16_t *cost, int16_t *hsum, int16_t *raw) {
    R3D_ROCTX_RANGE("r3d_sgbm_debug_fetch");
    if (!ctx) return R3D_E_BADARG;
    if (ctx->last_w == 0) return r3d_fail(ctx, R3D_E_BADARG, "debug_fetch: no sgbm call yet");
    if (ctx->last_w1 <= 0) return r3d_fail(ctx, R3D_E_BADARG, "debug_fetch: the last call had an empty matching range (all-invalid map), no volumes exist");
    R3D_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const size_t vol = (size_t)ctx->last_h * ctx->last_w1 * ctx->last_dp * 2;
    if (cost) R3D_HIP(ctx, hipMemcpy(cost, ctx->ws[0].cost.p, vol, hipMemcpyDeviceToHost));
    if (hsum) R3D_HIP(ctx, hipMemcpy(hsum, ctx->ws[0].hsum.p, vol, hipMemcpyDeviceToHost));
    if (raw) R3D_HIP(ctx, hipMemcpy(raw, ctx->ws[0].lrd.p, (size_t)ctx->last_w * ctx->last_h * 2, hipMemcpyDeviceToHost));
    return R3D_OK;
}

int r3d_sgbm_debug_hh_partial(r3d_ctx *ctx, int32_t n_dirs, int16_t *S_out) {
    R3D_ROCTX_RANGE("r3d_sgbm_debug_hh_partial");
    if (!ctx) return R3D_E_BADARG;
    if (ctx->last_w == 0) return r3d_fail(ctx, R3D_E_BADARG, "debug_hh_partial: no sgbm call yet");
    if (ctx->last_mode != R3D_SGBM_MODE_HH) return r3d_fail(ctx, R3D_E_BADARG, "debug_hh_partial: the last call was not MODE_HH (mode %d)", ctx->last_mode);
    if (ctx->last_w1 <= 0) return r3d_fail(ctx, R3D_E_BADARG, "debug_hh_partial: the last call had an empty matching range (all-invalid map), no volumes exist");
    if (n_dirs < 1 || n_dirs > 8) return r3d_fail(ctx, R3D_E_BADARG, "debug_hh_partial: n_dirs must be in 1..8, got %d", n_dirs);
    if (!S_out) return r3d_fail(ctx, R3D_E_BADARG, "debug_hh_partial: S_out is NULL");
    if (ctx->poisoned) return r3d_fail(ctx, R3D_E_HIP, "context poisoned by an earlier timed-out call: destroy it");
    if (int rc = r3d_sgm_hh_partial(ctx, n_dirs)) return rc;
    R3D_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const size_t vol = (size_t)ctx->last_h * ctx->last_w1 * ctx->last_dp * 2;
    R3D_HIP(ctx, hipMemcpy(S_out, ctx->ws[0].hsum.p, vol, hipMemcpyDeviceToHost));
    return R3D_OK;
}

int r3d_sgbm_debug_fetch_select(r3d_ctx *ctx, int16_t *raw_wta, int16_t *mins, int16_t *lrd) {
    R3D_ROCTX_RANGE("r3d_sgbm_debug_fetch_select");
    if (!ctx) return R3D_E_BADARG;
    if (ctx->last_w == 0) return r3d_fail(ctx, R3D_E_BADARG, "debug_fetch_select: no sgbm call yet");
    if (ctx->last_w1 <= 0) return r3d_fail(ctx, R3D_E_BADARG, "debug_fetch_select: the last call had an empty matching range (all-invalid map), no planes exist");
    R3D_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const size_t plane = (size_t)ctx->last_w * ctx->last_h * 2;
    if (raw_wta) R3D_HIP(ctx, hipMemcpy(raw_wta, ctx->ws[0].raw.p, plane, hipMemcpyDeviceToHost));
    if (mins) R3D_HIP(ctx, hipMemcpy(mins, ctx->ws[0].mins.p, plane, hipMemcpyDeviceToHost));
    if (lrd) R3D_HIP(ctx, hipMemcpy(lrd, ctx->ws[0].lrd.p, plane, hipMemcpyDeviceToHost));
    return R3D_OK;
}

int r3d_sgbm_debug_select(r3d_ctx *ctx, const r3d_sgbm_params *params, int32_t w, int32_t h, const int16_t *cost, const int16_t *cspec,
                          const int16_t *hsum, int32_t cost_pad, int32_t hsum_pad, int16_t *raw_out, int16_t *mins_out, int16_t *lrd_out) {
    R3D_ROCTX_RANGE("r3d_sgbm_debug_select");
    if (!ctx) return R3D_E_BADARG;
    if (int rc = r3d_sgm_debug_select(ctx, params, w, h, cost, cspec, hsum, cost_pad, hsum_pad)) return rc;
    return r3d_sgbm_debug_fetch_select(ctx, raw_out, mins_out, lrd_out);
}

}  // extern "C"
