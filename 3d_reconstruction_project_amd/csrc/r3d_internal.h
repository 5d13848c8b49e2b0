// Internal (not installed) declarations shared by the translation units of libr3d_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <atomic>
#include <cmath>
#include <initializer_list>
#include <string>
#include <vector>

#include "../../include/r3d.h"
#include "r3d_resources.h"

#define R3D_MAX_PROF 16
#define R3D_PIN_BYTES 65536
#define R3D_MAX_DEVICES 64   /* per-device caches of launch geometry */
#define R3D_PROF_SETS 4

struct r3d_prof_set {
    r3d_events<R3D_MAX_PROF + 1> ev;   // created at the first profiled call of the lane (r3d_prof_begin)
    const char *name[R3D_MAX_PROF] = {};
    int n = 0;
    bool pending = false;
};

#define R3D_SGM_MAX_LANES 6   /* workspaces that can exist; r3d_sgbm_compute_batch* uses R3D_SGM_LANES of them (env, default 3) */
#define R3D_SGM_LANES 3

// one SGM pipeline lane: its own grow-only workspace, stream and profiling event ring.  Single-map calls use lane 0 on
// the context stream; r3d_sgbm_compute_batch_dev spreads maps over the lanes so that kernels with complementary
// bottlenecks (cost: VALU + writes, hscan: HBM, vscan: mixed) of consecutive maps overlap.
struct r3d_sgm_ws {
    r3d_buf rec_l, rec_r, cost, cspec, hsum, ckpt, raw, mins, lrd, lrd2, flags, spk_l, spk_c;
    r3d_stream stream;
    r3d_event done;
    r3d_prof_set prof[R3D_PROF_SETS];
    int prof_cur = 0;
    bool ev_created = false;
};

// derived parameters of one sgbm call (sgm.hip: derive_geom), passed to every SGM kernel by value
struct SgmGeom {
    int W, H, minD, D, NP, minX1, maxX1, W1, SW2, SH2, P1, P2, uniq, d12, ftzero, stripe_sz, overlap, invalid;
    int DP;  // disparity slots per cost-volume column: the smallest of 32 / 64 / 128 / 256 / 512 that holds D
    int CN;  // channels of the image pair (1 grey, 3 colour: the block cost is the sum over the channels)
};

struct r3d_ctx {
    int device = 0;
    r3d_stream own_stream;
    hipStream_t stream = nullptr;   // own_stream, or the caller's (r3d_set_stream)
    std::string err;
    bool profiling = false;
    // set when a call gave up on work that is still queued on the stream (the registration loop's deadline): the arena and the
    // workspaces that work uses must not be handed to another call, so every later compute call on this ctx fails (R3D_E_HIP)
    // until it is destroyed
    bool poisoned = false;
    // grow-only workspace
    r3d_buf img_l, img_r, out;
    r3d_sgm_ws ws[R3D_SGM_MAX_LANES];
    r3d_event fork_ev;
    // geometry of the last sgbm call (for debug fetch)
    int last_w = 0, last_h = 0, last_w1 = 0, last_dp = 0;
    int last_mode = -1;        // r3d_sgbm_params.mode of that call
    SgmGeom last_geom = {};    // as its kernels saw it (MODE_HH: one stripe); r3d_sgbm_debug_hh_partial launches from it
    // profiling sums accumulate per kernel name over all lanes
    const char *acc_name[R3D_MAX_PROF] = {};
    double acc_ms[R3D_MAX_PROF] = {};
    int acc_cnt[R3D_MAX_PROF] = {};
    int n_acc = 0;
    // cloud workspace (cloud.hip)
    std::vector<r3d_buf> cloud_bufs;
    r3d_pinned icp_host;           // pinned landing buffer of the per-iteration sums
    unsigned pin_seq = 0;          // sequence number of the latest PinRead
    r3d_pinned pin;                // pinned landing buffer of the small device -> host reads between kernels (R3D_PIN_BYTES)
    // pre/post-processing workspace (prepost.hip)
    std::vector<r3d_buf> pp_bufs;
    r3d_buf pp_minmax, pp_lut;
    double pp_lut_sigma = -1.0;
    int pp_lut_n = 0;
};

// grows a context workspace buffer (all of them are grow-only and settle during warm-up)
static inline int r3d_reserve(r3d_ctx *ctx, r3d_buf &b, size_t bytes) { return b.reserve(ctx, ctx->stream, bytes, R3D_GROW_WORKSPACE); }

#define R3D_HIP(ctx, call)                                                                          \
    do {                                                                                            \
        hipError_t e_ = (call);                                                                     \
        if (e_ != hipSuccess)                                                                       \
            return r3d_fail((ctx), R3D_E_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), \
                            __FILE__, __LINE__);                                                    \
    } while (0)

struct DevArena {  // simple bump allocator over one of the context's buffer lists (grow-only, reused across calls)
    r3d_ctx *ctx;
    std::vector<r3d_buf> &bufs;   // ctx->cloud_bufs, or ctx->pp_bufs for the pre/post stages
    size_t next = 0;
    int rc = R3D_OK;
    explicit DevArena(r3d_ctx *c) : ctx(c), bufs(c->cloud_bufs) {}
    DevArena(r3d_ctx *c, std::vector<r3d_buf> &v) : ctx(c), bufs(v) {}
    void *get(size_t bytes) {
        if (rc) return nullptr;
        if (ctx->poisoned) {
            rc = r3d_fail(ctx, R3D_E_HIP, "context poisoned by an earlier timed-out call (its kernels may still use the arena): destroy it");
            return nullptr;
        }
        if (next >= bufs.size()) bufs.emplace_back();
        r3d_buf &b = bufs[next++];
        rc = r3d_reserve(ctx, b, bytes ? bytes : 16);
        return rc ? nullptr : b.p;
    }
};

// ---- staging around the device core of a host-buffer entry point: copies on ctx->stream, enqueued only (the entry point synchronises).
// host array -> fresh arena buffer; a null h gives a null *d and takes no arena slot, count == 0 takes a slot and copies nothing
template <class T>
int r3d_upload(r3d_ctx *ctx, DevArena &ar, const T *h, size_t count, const T **d) {
    *d = nullptr;
    if (!h) return R3D_OK;
    T *p = (T *)ar.get(count * sizeof(T));
    if (ar.rc) return ar.rc;
    if (count) R3D_HIP(ctx, hipMemcpyAsync(p, h, count * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
    *d = p;
    return R3D_OK;
}
// strided host image (rows of row_elems elements, stride_elems apart, both in elements of T) -> dense plane in a fresh arena buffer
template <class T>
int r3d_upload_plane(r3d_ctx *ctx, DevArena &ar, const T *h, int row_elems, int rows, size_t stride_elems, T **d) {
    const size_t row = (size_t)row_elems * sizeof(T);
    *d = (T *)ar.get(row * rows);
    if (ar.rc) return ar.rc;
    R3D_HIP(ctx, hipMemcpy2DAsync(*d, row, h, stride_elems * sizeof(T), row, rows, hipMemcpyHostToDevice, ctx->stream));
    return R3D_OK;
}
// device buffer -> host array; nothing for a null h (an output the caller did not ask for) or a zero count
template <class T>
int r3d_download(r3d_ctx *ctx, T *h, const T *d, size_t count) {
    if (h && count) R3D_HIP(ctx, hipMemcpyAsync(h, d, count * sizeof(T), hipMemcpyDeviceToHost, ctx->stream));
    return R3D_OK;
}
// the refusal of a count / capacity protocol: `have` rows of `what` against the caller's capacity
static inline int r3d_fits(r3d_ctx *ctx, const char *who, const char *what, int64_t have, int64_t cap) {
    return have <= cap ? R3D_OK : r3d_fail(ctx, R3D_E_BADARG, "%s: %lld %s do not fit a capacity of %lld", who, (long long)have, what, (long long)cap);
}
// the same for two quantities that are written together or not at all: one message with both counts when either does not fit
static inline int r3d_fits2(r3d_ctx *ctx, const char *who, const char *what_a, int64_t have_a, const char *what_b, int64_t have_b, int64_t cap_a,
                            int64_t cap_b) {
    if (have_a <= cap_a && have_b <= cap_b) return R3D_OK;
    return r3d_fail(ctx, R3D_E_BADARG, "%s: %lld %s and %lld %s do not fit capacities of %lld and %lld", who, (long long)have_a, what_a, (long long)have_b,
                    what_b, (long long)cap_a, (long long)cap_b);
}
// small device -> host reads between kernels: the copies in list order on ctx->stream (a null dev: an entry that is not read), then the
// call's one wait.  A HIP failure here reports this header's line, not the caller's: the entry point's roctx range names the call.
struct r3d_read { void *host; const void *dev; size_t bytes; };
static inline int r3d_read_back(r3d_ctx *ctx, std::initializer_list<r3d_read> reads) {
    for (const r3d_read &r : reads)
        if (r.dev) R3D_HIP(ctx, hipMemcpyAsync(r.host, r.dev, r.bytes, hipMemcpyDeviceToHost, ctx->stream));
    R3D_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return R3D_OK;
}

// 256-thread blocks for n items
static inline unsigned r3d_blocks(int64_t n) { return (unsigned)((n + 255) / 256); }

// the _dev forms refuse outputs that overlap an input or one another: a kernel would read rows another thread has already replaced.
// A null or empty span overlaps nothing; an output is tested against the inputs first, then against the outputs before it.
struct r3d_span { const void *p; size_t bytes; };
static inline int r3d_distinct(r3d_ctx *ctx, const char *who, const r3d_span *out, int n_out, const r3d_span *in, int n_in) {
    auto overlap = [](const r3d_span &a, const r3d_span &b) {
        if (!a.p || !b.p || !a.bytes || !b.bytes) return false;
        const uintptr_t a0 = (uintptr_t)a.p, b0 = (uintptr_t)b.p;
        return a0 < b0 + b.bytes && b0 < a0 + a.bytes;
    };
    for (int i = 0; i < n_out; i++) {
        for (int j = 0; j < n_in; j++)
            if (overlap(out[i], in[j])) return r3d_fail(ctx, R3D_E_BADARG, "%s: an output array overlaps an input array", who);
        for (int j = 0; j < i; j++)
            if (overlap(out[i], out[j])) return r3d_fail(ctx, R3D_E_BADARG, "%s: two output arrays overlap", who);
    }
    return R3D_OK;
}

// SolveJacobianSystemAndObtainExtrinsicMatrix: x = LDLT(JTJ) \ (-JTr); identity when |det| < det_tol (the registration loop's
// 1e-6).  det_tol < 0 (FGR: Open3D's SolveLinearSystemPSD has no such rule): no determinant test; the identity only for a zero
// pivot or a non-finite x.
__host__ __device__ inline bool solve6_to_matrix(const double *s, double U[16], double det_tol = 1e-6) {
    double A[6][6], b[6];
    for (int a = 0, q = 2; a < 6; a++)
        for (int c = a; c < 6; c++, q++) A[a][c] = A[c][a] = s[q];
    for (int a = 0; a < 6; a++) b[a] = -s[23 + a];
    // LDL^T
    double L[6][6], Dg[6];
    for (int i = 0; i < 6; i++) for (int j = 0; j < 6; j++) L[i][j] = 0;
    double det = 1;
    for (int j = 0; j < 6; j++) {
        double d = A[j][j];
        for (int k = 0; k < j; k++) d -= L[j][k] * L[j][k] * Dg[k];
        Dg[j] = d;
        det *= d;
        L[j][j] = 1;
        for (int i = j + 1; i < 6; i++) {
            double v = A[i][j];
            for (int k = 0; k < j; k++) v -= L[i][k] * L[j][k] * Dg[k];
            L[i][j] = d != 0 ? v / d : 0;
        }
    }
    for (int i = 0; i < 16; i++) U[i] = (i % 5 == 0);
    if (det_tol >= 0) {
        if (!isfinite(det) || fabs(det) < det_tol) return false;
    } else {
        for (int j = 0; j < 6; j++) if (Dg[j] == 0) return false;
    }
    double y[6], x[6];
    for (int i = 0; i < 6; i++) { y[i] = b[i]; for (int k = 0; k < i; k++) y[i] -= L[i][k] * y[k]; }
    for (int i = 0; i < 6; i++) y[i] /= Dg[i];
    for (int i = 5; i >= 0; i--) { x[i] = y[i]; for (int k = i + 1; k < 6; k++) x[i] -= L[k][i] * x[k]; }
    if (det_tol < 0) {
        for (int i = 0; i < 6; i++) if (!isfinite(x[i])) return false;
    }
    // TransformVector6dToMatrix4d: R = Rz(x2) Ry(x1) Rx(x0)
    double ca, sa, cb, sb, cc, sc;   // one range reduction per angle (the update runs in a single GPU thread)
    sincos(x[0], &sa, &ca);
    sincos(x[1], &sb, &cb);
    sincos(x[2], &sc, &cc);
    const double R[9] = {cc * cb, cc * sb * sa - sc * ca, cc * sb * ca + sc * sa, sc * cb, sc * sb * sa + cc * ca, sc * sb * ca - cc * sa,
                         -sb, cb * sa, cb * ca};
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) U[i * 4 + j] = R[i * 3 + j];
        U[i * 4 + 3] = x[3 + i];
    }
    return true;
}

// profiling helpers: record an event before each named kernel when ctx->profiling
void r3d_prof_harvest(r3d_ctx *ctx, r3d_prof_set &ps);
static inline void r3d_prof_begin(r3d_ctx *ctx, r3d_sgm_ws &ws) {
    if (!ctx->profiling) return;
    if (!ws.ev_created) {
        for (auto &ps : ws.prof)
            for (int i = 0; i <= R3D_MAX_PROF; i++) (void)ps.ev.create(i);
        ws.ev_created = true;
    }
    ws.prof_cur = (ws.prof_cur + 1) % R3D_PROF_SETS;
    r3d_prof_set &ps = ws.prof[ws.prof_cur];
    if (ps.pending) r3d_prof_harvest(ctx, ps);
    ps.n = 0;
}
static inline void r3d_prof_mark(r3d_ctx *ctx, r3d_sgm_ws &ws, hipStream_t st, const char *name) {
    if (!ctx->profiling) return;
    r3d_prof_set &ps = ws.prof[ws.prof_cur];
    if (ps.n >= R3D_MAX_PROF) return;
    (void)hipEventRecord(ps.ev[ps.n], st);
    ps.name[ps.n] = name;
    ps.n++;
}
static inline void r3d_prof_end(r3d_ctx *ctx, r3d_sgm_ws &ws, hipStream_t st) {
    if (!ctx->profiling) return;
    r3d_prof_set &ps = ws.prof[ws.prof_cur];
    (void)hipEventRecord(ps.ev[ps.n], st);
    ps.pending = true;
}


// roctx ranges around every C-ABI entry point ("rocprofv3 --marker-trace attributes kernels to entry
// points").  The marker library is looked up at run time (librocprofiler-sdk-roctx.so, the one rocprofv3 listens to, else the
// legacy libroctx64.so); without it, or with R3D_ROCTX=0, a range is two predictable branches.
bool r3d_roctx_push(const char *name);   // true if a range was opened (the scope pops only then: contexts live on several threads)
void r3d_roctx_pop();
struct r3d_roctx_scope {
    bool pushed;
    explicit r3d_roctx_scope(const char *name) : pushed(r3d_roctx_push(name)) {}
    ~r3d_roctx_scope() { if (pushed) r3d_roctx_pop(); }
    r3d_roctx_scope(const r3d_roctx_scope &) = delete;
    r3d_roctx_scope &operator=(const r3d_roctx_scope &) = delete;
};
#define R3D_ROCTX_RANGE(name) r3d_roctx_scope r3d_roctx_scope_(name)

// sgm.hip
int r3d_sgm_run(r3d_ctx *ctx, int lane, hipStream_t st, const r3d_sgbm_params *p, const uint8_t *d_left, const uint8_t *d_right,
                int w, int h, int stride, int cn, int16_t *d_disp);
int r3d_sgm_hh_partial(r3d_ctx *ctx, int n_dirs);
int r3d_sgm_debug_select(r3d_ctx *ctx, const r3d_sgbm_params *p, int w, int h, const int16_t *cost, const int16_t *cspec,
                         const int16_t *hsum, int cost_pad, int hsum_pad);
int r3d_selftest_run(r3d_ctx *ctx);
int r3d_speckle_run(r3d_ctx *ctx, r3d_sgm_ws &ws, hipStream_t st, int16_t *d_img, int w, int h, int newVal, int maxSize, int maxDiff);
int r3d_streambench_run(r3d_ctx *ctx, int mode, int rows, size_t row_bytes, int write, int delay, int reps, float *ms);

// cloud.hip: exclusive scan of n ints on the ctx stream (in and out 16-byte aligned and distinct; tiles of 4096 elements)
int r3d_exclusive_scan_i32(r3d_ctx *ctx, DevArena &ar, const int *in, int *out, int64_t n);
// cloud.hip: point numbers in the stable order of their voxel key (cx * dims[1] + cy) * dims[2] + cz, c = clamp(floor((p - org) / cell))
int r3d_sort_by_voxel_u32(r3d_ctx *ctx, DevArena &ar, const double *d_pts, int64_t n, const double org[3], double cell, const int dims[3],
                          const unsigned **keys_sorted, const int **idx_sorted);
// cloud.hip: the stable LSD radix sort (eight bits per pass) of n (uint64 key, int32 value) pairs whose keys are below 2^bits; values
// default to the index (d_vals null).  Inputs are only read, results are arena buffers, all on the ctx stream without a host round
// trip.  A key wider than 64 bits is sorted by chaining calls, least significant part first, the next part gathered through the values.
int r3d_sort_pairs_u64(r3d_ctx *ctx, DevArena &ar, const uint64_t *d_keys, const int *d_vals, int64_t n, int bits, const uint64_t **keys_sorted,
                       const int **vals_sorted);
