// Triangle-mesh operations on the device ("Triangle-mesh operations"; C ABI: r3d_trimesh_*): vertex/triangle
// incidence and vertex adjacency in a fixed order, the three smoothing filters of Open3D's TriangleMesh, triangle and vertex
// normals, and the clean-ups that compact vertices and triangles.  tests/trimesh_ref.py restates every result in numpy.
//
// Order is what makes the floating-point results unique: a vertex's incidence list holds its corners 3 t + c ascending, its
// adjacency list its neighbours ascending without repeats, and every sum walks one of the two from the front.  Atomics only count
// and hand out slots; every segment they fill is sorted afterwards, so their arrival order never reaches a result.
#include "r3d_mesh.h"

#include <climits>

namespace {

constexpr int TM_SHORT = 32;    // a vertex in at most this many corners: one thread sorts its segments by insertion (typical: 6)
constexpr int TM_LDS = 4096;    // longer segments are sorted by a workgroup: in LDS up to this many entries, in place beyond
// The one deliberate deviation from Open3D, which divides 0 / 0 for a vertex whose adjacency set is empty: such a vertex and its
// attributes are kept as they are.
constexpr bool TM_KEEP_ISOLATED = true;

struct TmHdr { int bad_index, n_long, pad0, pad1; };

// ---- incidence ----------------------------------------------------------------------------------------------------------------------
// one thread per corner: an index outside [0, nv) raises the flag and is not used; the others are counted per vertex
__global__ void __launch_bounds__(256) k_tm_count(const int32_t *__restrict__ tri, int64_t n3, int nv, int *__restrict__ count, TmHdr *__restrict__ hdr) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n3) return;
    const int v = tri[i];
    if ((unsigned)v >= (unsigned)nv) { hdr->bad_index = 1; return; }
    atomicAdd(&count[v], 1);
}

__global__ void __launch_bounds__(256) k_tm_classify(const int *__restrict__ count, int nv, int *__restrict__ long_list, TmHdr *__restrict__ hdr) {
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= nv) return;
    if (count[v] > TM_SHORT) long_list[atomicAdd(&hdr->n_long, 1)] = v;
}

// runs after the host has seen bad_index == 0: every index is a valid address
__global__ void __launch_bounds__(256) k_tm_fill(const int32_t *__restrict__ tri, int64_t n3, const int *__restrict__ inc_off, int *__restrict__ cursor,
                                                 int *__restrict__ inc) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n3) return;
    const int v = tri[i];
    inc[inc_off[v] + atomicAdd(&cursor[v], 1)] = (int)i;
}

// segment v of data is [off[v] * mul, off[v + 1] * mul): mul = 1 for the corners, 2 for the neighbour candidates
__global__ void __launch_bounds__(256) k_tm_sort_short(const int *__restrict__ off, int nv, int mul, int *__restrict__ data) {
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= nv) return;
    const int n = off[v + 1] - off[v];
    if (n > TM_SHORT) return;
    int *a = data + (int64_t)off[v] * mul;
    const int L = n * mul;
    for (int i = 1; i < L; i++) {
        const int x = a[i];
        int j = i - 1;
        while (j >= 0 && a[j] > x) { a[j + 1] = a[j]; j--; }
        a[j + 1] = x;
    }
}

__device__ __forceinline__ void tm_order(int *s, int64_t i, int64_t j) {
    const int a = s[i], b = s[j];
    if (a > b) { s[i] = b; s[j] = a; }
}

// one workgroup per long segment.  A bitonic network whose exchanges all put the smaller value at the lower index (the first
// step of a merge mirrors the upper half), so entries past the end behave as +infinity that never moves and any length sorts.
__global__ void __launch_bounds__(256) k_tm_sort_long(const int *__restrict__ off, const int *__restrict__ long_list, int mul, int *__restrict__ data) {
    __shared__ int lds[TM_LDS];
    const int v = long_list[blockIdx.x];
    int *a = data + (int64_t)off[v] * mul;
    const int L = (off[v + 1] - off[v]) * mul;
    const bool in_lds = L <= TM_LDS;
    if (in_lds) {
        for (int i = threadIdx.x; i < L; i += 256) lds[i] = a[i];
        __syncthreads();
    }
    int *s = in_lds ? lds : a;
    int lp = 1;
    while (((int64_t)1 << lp) < L) lp++;
    const int half = 1 << (lp - 1);   // pairs per step; the indices are 64-bit because the padded length can be 2^31
    for (int lk = 1; lk <= lp; lk++) {
        const int64_t k = (int64_t)1 << lk;
        for (int p = threadIdx.x; p < half; p += 256) {
            const int64_t base = (int64_t)(p >> (lk - 1)) << lk, r = p & ((k >> 1) - 1);
            const int64_t j = base + k - 1 - r;
            if (j < L) tm_order(s, base + r, j);
        }
        __syncthreads();
        for (int lj = lk - 2; lj >= 0; lj--) {
            const int64_t d = (int64_t)1 << lj;
            for (int p = threadIdx.x; p < half; p += 256) {
                const int64_t i = ((int64_t)(p >> lj) << (lj + 1)) + (p & (d - 1));
                if (i + d < L) tm_order(s, i, i + d);
            }
            __syncthreads();
        }
    }
    if (in_lds)
        for (int i = threadIdx.x; i < L; i += 256) a[i] = lds[i];
}

// ---- adjacency ----------------------------------------------------------------------------------------------------------------------
// entry e of the incidence list is corner c of triangle t: the two other vertices of t are candidates 2 e and 2 e + 1 of the same vertex
__global__ void __launch_bounds__(256) k_tm_candidates(const int32_t *__restrict__ tri, const int *__restrict__ inc, int64_t n3, int *__restrict__ cand) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n3) return;
    const int c = inc[e], t = c / 3, k = c - 3 * t;
    cand[2 * e] = tri[3 * (int64_t)t + (k == 2 ? 0 : k + 1)];
    cand[2 * e + 1] = tri[3 * (int64_t)t + (k == 0 ? 2 : k - 1)];
}

// the sorted candidates of a vertex without repeats: counted (WRITE false), then written behind adj_off[v]
template <bool WRITE>
__global__ void __launch_bounds__(256) k_tm_unique(const int *__restrict__ inc_off, const int *__restrict__ cand, int nv, int *__restrict__ adj_cnt,
                                                   const int *__restrict__ adj_off, int *__restrict__ adj) {
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= nv) return;
    const int64_t b = 2 * (int64_t)inc_off[v], e = 2 * (int64_t)inc_off[v + 1];
    int n = 0, last = -1;   // vertex numbers are >= 0
    int *out = WRITE ? adj + adj_off[v] : nullptr;
    for (int64_t j = b; j < e; j++) {
        const int x = cand[j];
        if (x != last) {
            if (WRITE) out[n] = x;
            n++;
            last = x;
        }
    }
    if (!WRITE) adj_cnt[v] = n;
}

// ---- smoothing ----------------------------------------------------------------------------------------------------------------------
template <int NA> struct TmAttrs { const double *src[NA]; double *dst[NA]; };

// one step of filter_smooth_simple (LAPLACE false) or filter_smooth_laplacian, one thread per vertex, for NA attribute arrays at
// once; the weights of the Laplacian step always come from pos, the positions the step starts from
template <bool LAPLACE, int NA>
__global__ void __launch_bounds__(256) k_tm_smooth(const int *__restrict__ adj_off, const int *__restrict__ adj, int nv, double lambda,
                                                   const double *__restrict__ pos, TmAttrs<NA> A) {
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= nv) return;
    const int b = adj_off[v], e = adj_off[v + 1];
    double own[NA][3], acc[NA][3];
#pragma unroll
    for (int a = 0; a < NA; a++)
#pragma unroll
        for (int c = 0; c < 3; c++) {
            own[a][c] = A.src[a][3 * (int64_t)v + c];
            acc[a][c] = LAPLACE ? 0.0 : own[a][c];
        }
    if (TM_KEEP_ISOLATED && e == b) {
#pragma unroll
        for (int a = 0; a < NA; a++)
#pragma unroll
            for (int c = 0; c < 3; c++) A.dst[a][3 * (int64_t)v + c] = own[a][c];
        return;
    }
    const double p0 = pos[3 * (int64_t)v], p1 = pos[3 * (int64_t)v + 1], p2 = pos[3 * (int64_t)v + 2];
    double tw = 0.0;
    for (int j = b; j < e; j++) {
        const int64_t nb = 3 * (int64_t)adj[j];
        double w = 1.0;
        if (LAPLACE) {
            const double d0 = p0 - pos[nb], d1 = p1 - pos[nb + 1], d2 = p2 - pos[nb + 2];
            const double dist = sqrt((d0 * d0 + d1 * d1) + d2 * d2);
            w = 1.0 / (dist + 1e-12);
            tw += w;
        }
#pragma unroll
        for (int a = 0; a < NA; a++)
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const double x = A.src[a][nb + c];
                acc[a][c] += LAPLACE ? w * x : x;
            }
    }
    const double div = LAPLACE ? tw : (double)(e - b + 1);
#pragma unroll
    for (int a = 0; a < NA; a++)
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const double m = acc[a][c] / div;
            A.dst[a][3 * (int64_t)v + c] = LAPLACE ? own[a][c] + lambda * (m - own[a][c]) : m;
        }
}

// ---- normals ------------------------------------------------------------------------------------------------------------------------
// (v1 - v0) x (v2 - v0) in the order numpy's cross writes it
__device__ __forceinline__ void tm_face(const double *__restrict__ pos, const int32_t *__restrict__ tri, int64_t t, double n[3]) {
    const int64_t i0 = 3 * (int64_t)tri[3 * t], i1 = 3 * (int64_t)tri[3 * t + 1], i2 = 3 * (int64_t)tri[3 * t + 2];
    const double a0 = pos[i1] - pos[i0], a1 = pos[i1 + 1] - pos[i0 + 1], a2 = pos[i1 + 2] - pos[i0 + 2];
    const double b0 = pos[i2] - pos[i0], b1 = pos[i2 + 1] - pos[i0 + 1], b2 = pos[i2 + 2] - pos[i0 + 2];
    n[0] = a1 * b2 - a2 * b1;
    n[1] = a2 * b0 - a0 * b2;
    n[2] = a0 * b1 - a1 * b0;
}
__device__ __forceinline__ void tm_store_normal(double *__restrict__ out, int64_t row, double n[3], bool raw) {
    if (!raw) {
        const double len = sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
        if (len != 0.0) { n[0] = n[0] / len; n[1] = n[1] / len; n[2] = n[2] / len; }   // a zero vector stays zero
    }
    out[3 * row] = n[0]; out[3 * row + 1] = n[1]; out[3 * row + 2] = n[2];
}

__global__ void __launch_bounds__(256) k_tm_triangle_normals(const double *__restrict__ pos, const int32_t *__restrict__ tri, int64_t nt, int raw,
                                                             double *__restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= nt) return;
    double n[3];
    tm_face(pos, tri, t, n);
    tm_store_normal(out, t, n, raw != 0);
}

// the cross products of the vertex's triangles added from zero in ascending corner order
__global__ void __launch_bounds__(256) k_tm_vertex_normals(const double *__restrict__ pos, const int32_t *__restrict__ tri, const int *__restrict__ inc_off,
                                                           const int *__restrict__ inc, int nv, int raw, double *__restrict__ out) {
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= nv) return;
    double s[3] = {0.0, 0.0, 0.0};
    for (int j = inc_off[v]; j < inc_off[v + 1]; j++) {
        double n[3];
        tm_face(pos, tri, inc[j] / 3, n);
        s[0] += n[0]; s[1] += n[1]; s[2] += n[2];
    }
    tm_store_normal(out, v, s, raw != 0);
}

// ---- compaction ---------------------------------------------------------------------------------------------------------------------
// gone[v] = 1 for a vertex the caller's mask or the non-finite rule removes
__global__ void __launch_bounds__(256) k_tm_vertex_gone(const double *__restrict__ pos, const uint8_t *__restrict__ keep, int nv, int drop_non_finite,
                                                        int *__restrict__ gone) {
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= nv) return;
    int g = keep ? keep[v] == 0 : 0;
    if (drop_non_finite) g |= !(isfinite(pos[3 * (int64_t)v]) && isfinite(pos[3 * (int64_t)v + 1]) && isfinite(pos[3 * (int64_t)v + 2]));
    gone[v] = g;
}

// triangles are decided first: the caller's mask, the degenerate rule, and no corner at a removed vertex.  A surviving triangle
// marks its vertices as referenced.  An index outside [0, nv) raises the flag; the loads go to a clamped address.
__global__ void __launch_bounds__(256) k_tm_triangle_keep(const int32_t *__restrict__ tri, const uint8_t *__restrict__ keep, int64_t nt, int nv,
                                                          int drop_degenerate, const int *__restrict__ gone, int *__restrict__ tkeep, int *__restrict__ ref,
                                                          TmHdr *__restrict__ hdr) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= nt) return;
    const int a = tri[3 * t], b = tri[3 * t + 1], c = tri[3 * t + 2];
    const bool ok = (unsigned)a < (unsigned)nv && (unsigned)b < (unsigned)nv && (unsigned)c < (unsigned)nv;
    if (!ok) hdr->bad_index = 1;
    const int ca = ok ? a : 0, cb = ok ? b : 0, cc = ok ? c : 0;
    int k = keep ? keep[t] != 0 : 1;
    if (drop_degenerate) k &= !(a == b || b == c || a == c);
    k &= !(gone[ca] | gone[cb] | gone[cc]);
    k &= ok;
    tkeep[t] = k;
    if (k) { ref[ca] = 1; ref[cb] = 1; ref[cc] = 1; }
}

__global__ void __launch_bounds__(256) k_tm_vertex_keep(const int *__restrict__ gone, const int *__restrict__ ref, int nv, int drop_unreferenced,
                                                        int *__restrict__ vkeep) {
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= nv) return;
    vkeep[v] = !gone[v] && (!drop_unreferenced || ref[v]);
}

__global__ void __launch_bounds__(256) k_tm_scatter_rows(const int *__restrict__ keep, const int *__restrict__ map, int nv, const double *__restrict__ src,
                                                         double *__restrict__ dst) {
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= nv || !keep[v]) return;
    const int64_t o = 3 * (int64_t)map[v], i = 3 * (int64_t)v;
    dst[o] = src[i]; dst[o + 1] = src[i + 1]; dst[o + 2] = src[i + 2];
}

__global__ void __launch_bounds__(256) k_tm_scatter_triangles(const int *__restrict__ tkeep, const int *__restrict__ tmap, const int *__restrict__ vmap,
                                                              const int32_t *__restrict__ tri, int64_t nt, int32_t *__restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= nt || !tkeep[t]) return;
    const int64_t o = 3 * (int64_t)tmap[t];
    out[o] = vmap[tri[3 * t]]; out[o + 1] = vmap[tri[3 * t + 1]]; out[o + 2] = vmap[tri[3 * t + 2]];
}

// ====================================================================================================================== host side
struct TmTopo {
    int *inc_off = nullptr, *inc = nullptr;   // [nv + 1], [3 nt]
    int *adj_off = nullptr, *adj = nullptr;   // [nv + 1], [<= 6 nt]
};

int tm_sort_segments(r3d_ctx *ctx, const int *off, int nv, const int *long_list, int n_long, int mul, int *data) {
    k_tm_sort_short<<<r3d_blocks(nv), 256, 0, ctx->stream>>>(off, nv, mul, data);
    if (n_long) k_tm_sort_long<<<(unsigned)n_long, 256, 0, ctx->stream>>>(off, long_list, mul, data);
    R3D_HIP(ctx, hipGetLastError());
    return R3D_OK;
}

// what a caller needs of the lists: the index check alone (the count pass), the incidence, or the adjacency as well
enum TmLevel { TM_CHECK, TM_INCIDENCE, TM_ADJACENCY };

// the lists of nv > 0 vertices up to `level` on the context stream; fails R3D_E_BADARG on an index outside [0, nv) before anything
// is addressed by one.  One host read (the flag and the number of long segments).
int tm_topology(r3d_ctx *ctx, DevArena &ar, const char *who, int nv, int64_t nt, const int32_t *d_tri, TmLevel level, TmTopo &T) {
    hipStream_t st = ctx->stream;
    const int64_t n3 = 3 * nt;
    int *count = (int *)ar.get((size_t)(nv + 1) * 4 * 2);   // counts, then the fill cursors
    int *cursor = count + (nv + 1);
    T.inc_off = (int *)ar.get((size_t)(nv + 1) * 4);
    T.inc = (int *)ar.get((size_t)n3 * 4);
    int *long_list = (int *)ar.get((size_t)nv * 4);
    TmHdr *hdr = (TmHdr *)ar.get(sizeof(TmHdr));
    if (ar.rc) return ar.rc;
    R3D_HIP(ctx, hipMemsetAsync(count, 0, (size_t)(nv + 1) * 4 * 2, st));
    R3D_HIP(ctx, hipMemsetAsync(hdr, 0, sizeof(TmHdr), st));
    if (nt) k_tm_count<<<r3d_blocks(n3), 256, 0, st>>>(d_tri, n3, nv, count, hdr);
    k_tm_classify<<<r3d_blocks(nv), 256, 0, st>>>(count, nv, long_list, hdr);
    R3D_HIP(ctx, hipGetLastError());
    if (int rc = r3d_exclusive_scan_i32(ctx, ar, count, T.inc_off, (int64_t)nv + 1)) return rc;
    TmHdr h = {};
    if (int rc = r3d_read_back(ctx, {{&h, hdr, sizeof(TmHdr)}})) return rc;
    if (h.bad_index) return r3d_fail(ctx, R3D_E_BADARG, "%s: a triangle index outside [0, %d)", who, nv);
    if (level == TM_CHECK) return R3D_OK;
    if (nt) {
        k_tm_fill<<<r3d_blocks(n3), 256, 0, st>>>(d_tri, n3, T.inc_off, cursor, T.inc);
        if (int rc = tm_sort_segments(ctx, T.inc_off, nv, long_list, h.n_long, 1, T.inc)) return rc;
    }
    if (level == TM_INCIDENCE) return R3D_OK;
    int *cand = (int *)ar.get((size_t)n3 * 2 * 4);
    int *adj_cnt = (int *)ar.get((size_t)(nv + 1) * 4);
    T.adj_off = (int *)ar.get((size_t)(nv + 1) * 4);
    T.adj = (int *)ar.get((size_t)n3 * 2 * 4);
    if (ar.rc) return ar.rc;
    if (nt) {
        k_tm_candidates<<<r3d_blocks(n3), 256, 0, st>>>(d_tri, T.inc, n3, cand);
        if (int rc = tm_sort_segments(ctx, T.inc_off, nv, long_list, h.n_long, 2, cand)) return rc;
    }
    R3D_HIP(ctx, hipMemsetAsync(adj_cnt + nv, 0, 4, st));
    k_tm_unique<false><<<r3d_blocks(nv), 256, 0, st>>>(T.inc_off, cand, nv, adj_cnt, nullptr, nullptr);
    R3D_HIP(ctx, hipGetLastError());
    if (int rc = r3d_exclusive_scan_i32(ctx, ar, adj_cnt, T.adj_off, (int64_t)nv + 1)) return rc;
    k_tm_unique<true><<<r3d_blocks(nv), 256, 0, st>>>(T.inc_off, cand, nv, nullptr, T.adj_off, T.adj);
    R3D_HIP(ctx, hipGetLastError());
    return R3D_OK;
}

// the lists on the host: the count always, offsets and entries when cap allows
int tm_lists(r3d_ctx *ctx, const char *who, bool adjacency, int64_t nv, int64_t nt, const int32_t *triangles, int64_t cap, int32_t *offsets, int32_t *list,
             int64_t *out_n) {
    if (int rc = r3d_mesh_sizes_ok(ctx, who, nv, nt)) return rc;
    if (!out_n || cap < 0 || (nt > 0 && !triangles) || (cap > 0 && (!offsets || !list)))
        return r3d_fail(ctx, R3D_E_BADARG, "%s: a missing array or a negative capacity", who);
    *out_n = 0;
    R3D_HIP(ctx, hipSetDevice(ctx->device));
    if (int rc = r3d_mesh_empty_ok(ctx, who, nv, nt)) return rc;
    if (nv == 0) {
        if (cap > 0) offsets[0] = 0;
        return R3D_OK;
    }
    DevArena ar(ctx);
    const int32_t *d_tri;
    if (int rc = r3d_upload(ctx, ar, triangles, (size_t)nt * 3, &d_tri)) return rc;
    TmTopo T;
    if (int rc = tm_topology(ctx, ar, who, (int)nv, nt, d_tri, adjacency ? TM_ADJACENCY : TM_INCIDENCE, T)) return rc;
    const int *d_off = adjacency ? T.adj_off : T.inc_off, *d_list = adjacency ? T.adj : T.inc;
    int total = 0;
    if (int rc = r3d_read_back(ctx, {{&total, d_off + nv, 4}})) return rc;
    *out_n = total;
    if (cap == 0) return R3D_OK;
    if (int rc = r3d_fits(ctx, who, "entries", total, cap)) return rc;
    if (int rc = r3d_download(ctx, offsets, d_off, (size_t)nv + 1)) return rc;
    if (int rc = r3d_download(ctx, list, d_list, (size_t)total)) return rc;
    R3D_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return R3D_OK;
}

// ---- smoothing ----------------------------------------------------------------------------------------------------------------------
struct TmSmooth {
    int64_t nv, nt;
    r3d_mesh_in in;     // device; nrm / col may be null
    int kind, iterations, scope;
    double lambda, mu;
    r3d_mesh_out out;   // no triangles
};

int tm_smooth_args_ok(r3d_ctx *ctx, int64_t nv, int64_t nt, const void *vertices, const void *normals, const void *colors, const void *triangles, int kind,
                      int iterations, double lambda, double mu, int scope, const void *out_vertices, const void *out_normals, const void *out_colors) {
    if (int rc = r3d_mesh_sizes_ok(ctx, "trimesh_smooth", nv, nt)) return rc;
    if (iterations < 0) return r3d_fail(ctx, R3D_E_BADARG, "trimesh_smooth: %d iterations", iterations);
    if (iterations > R3D_SMOOTH_MAX_ITERATIONS)   // every step is a launch
        return r3d_fail(ctx, R3D_E_UNSUPPORTED, "trimesh_smooth: %d iterations, more than %d", iterations, R3D_SMOOTH_MAX_ITERATIONS);
    if (kind != R3D_SMOOTH_SIMPLE && kind != R3D_SMOOTH_LAPLACIAN && kind != R3D_SMOOTH_TAUBIN)
        return r3d_fail(ctx, R3D_E_BADARG, "trimesh_smooth: unknown kind %d", kind);
    if (scope != R3D_SCOPE_ALL && scope != R3D_SCOPE_COLOR && scope != R3D_SCOPE_NORMAL && scope != R3D_SCOPE_VERTEX)
        return r3d_fail(ctx, R3D_E_BADARG, "trimesh_smooth: unknown scope %d", scope);
    if (!std::isfinite(lambda) || !std::isfinite(mu)) return r3d_fail(ctx, R3D_E_BADARG, "trimesh_smooth: lambda and mu must be finite");
    if ((nv > 0 && (!vertices || !out_vertices || (normals && !out_normals) || (colors && !out_colors))) || (nt > 0 && !triangles))
        return r3d_fail(ctx, R3D_E_BADARG, "trimesh_smooth: a missing array");
    return R3D_OK;
}

template <bool LAPLACE, int NA>
void tm_launch_smooth(hipStream_t st, const TmTopo &T, int nv, double lambda, const double *pos, const double *const src[3], double *const dst[3]) {
    TmAttrs<NA> A;
    for (int a = 0; a < NA; a++) { A.src[a] = src[a]; A.dst[a] = dst[a]; }
    k_tm_smooth<LAPLACE, NA><<<r3d_blocks(nv), 256, 0, st>>>(T.adj_off, T.adj, nv, lambda, pos, A);
}

// device arrays in and out.  Step k of S writes the caller's output arrays when S - k is even and arena copies otherwise, so the
// last step lands in the outputs; the first step reads the inputs.
int tm_smooth(r3d_ctx *ctx, DevArena &ar, const TmSmooth &m) {
    hipStream_t st = ctx->stream;
    if (int rc = r3d_mesh_empty_ok(ctx, "trimesh_smooth", m.nv, m.nt)) return rc;
    if (m.nv == 0) return R3D_OK;
    const int nv = (int)m.nv;
    const size_t bytes = (size_t)nv * 24;
    TmTopo T;
    if (int rc = tm_topology(ctx, ar, "trimesh_smooth", nv, m.nt, m.in.tri, TM_ADJACENCY, T)) return rc;
    // the filtered attributes, positions first
    const bool f_pos = m.scope == R3D_SCOPE_ALL || m.scope == R3D_SCOPE_VERTEX;
    const bool f_nrm = m.in.nrm && (m.scope == R3D_SCOPE_ALL || m.scope == R3D_SCOPE_NORMAL);
    const bool f_col = m.in.col && (m.scope == R3D_SCOPE_ALL || m.scope == R3D_SCOPE_COLOR);
    const double *in[3] = {};
    double *out[3] = {}, *tmp[3] = {};
    int na = 0;
    if (f_pos) { in[na] = m.in.pos; out[na++] = m.out.pos; }
    if (f_nrm) { in[na] = m.in.nrm; out[na++] = m.out.nrm; }
    if (f_col) { in[na] = m.in.col; out[na++] = m.out.col; }
    const int steps = m.kind == R3D_SMOOTH_TAUBIN ? 2 * m.iterations : m.iterations;   // at most 2 R3D_SMOOTH_MAX_ITERATIONS
    const bool filtering = steps > 0 && na > 0;
    // what is not filtered is copied
    if (!(filtering && f_pos)) R3D_HIP(ctx, hipMemcpyAsync(m.out.pos, m.in.pos, bytes, hipMemcpyDeviceToDevice, st));
    if (m.in.nrm && !(filtering && f_nrm)) R3D_HIP(ctx, hipMemcpyAsync(m.out.nrm, m.in.nrm, bytes, hipMemcpyDeviceToDevice, st));
    if (m.in.col && !(filtering && f_col)) R3D_HIP(ctx, hipMemcpyAsync(m.out.col, m.in.col, bytes, hipMemcpyDeviceToDevice, st));
    if (!filtering) return R3D_OK;
    if (steps > 1) {
        for (int a = 0; a < na; a++) tmp[a] = (double *)ar.get(bytes);
        if (ar.rc) return ar.rc;
    }
    const double *src[3] = {in[0], in[1], in[2]};
    for (int k = 1; k <= steps; k++) {
        double *const *dst = (steps - k) % 2 == 0 ? out : tmp;
        const double *pos = f_pos ? src[0] : m.in.pos;   // the positions this step starts from
        const double lam = m.kind == R3D_SMOOTH_TAUBIN && k % 2 == 0 ? m.mu : m.lambda;
        if (m.kind == R3D_SMOOTH_SIMPLE) {
            if (na == 1) tm_launch_smooth<false, 1>(st, T, nv, lam, pos, src, dst);
            else if (na == 2) tm_launch_smooth<false, 2>(st, T, nv, lam, pos, src, dst);
            else tm_launch_smooth<false, 3>(st, T, nv, lam, pos, src, dst);
        } else {
            if (na == 1) tm_launch_smooth<true, 1>(st, T, nv, lam, pos, src, dst);
            else if (na == 2) tm_launch_smooth<true, 2>(st, T, nv, lam, pos, src, dst);
            else tm_launch_smooth<true, 3>(st, T, nv, lam, pos, src, dst);
        }
        for (int a = 0; a < na; a++) src[a] = dst[a];
    }
    R3D_HIP(ctx, hipGetLastError());
    return R3D_OK;
}

// ---- normals ------------------------------------------------------------------------------------------------------------------------
int tm_normals_args_ok(r3d_ctx *ctx, int64_t nv, int64_t nt, const void *vertices, const void *triangles, int flags) {
    if (int rc = r3d_mesh_sizes_ok(ctx, "trimesh_normals", nv, nt)) return rc;
    if (flags & ~R3D_NORMALS_RAW) return r3d_fail(ctx, R3D_E_BADARG, "trimesh_normals: unknown flags %d", flags);
    if ((nv > 0 && !vertices) || (nt > 0 && !triangles)) return r3d_fail(ctx, R3D_E_BADARG, "trimesh_normals: a missing array");
    return R3D_OK;
}

int tm_normals(r3d_ctx *ctx, DevArena &ar, int64_t nv, int64_t nt, const double *d_pos, const int32_t *d_tri, int flags, double *d_tn, double *d_vn) {
    hipStream_t st = ctx->stream;
    if (int rc = r3d_mesh_empty_ok(ctx, "trimesh_normals", nv, nt)) return rc;
    if (nv == 0) return R3D_OK;
    TmTopo T;   // triangle normals alone need the index check, not the lists
    if (int rc = tm_topology(ctx, ar, "trimesh_normals", (int)nv, nt, d_tri, d_vn ? TM_INCIDENCE : TM_CHECK, T)) return rc;
    const int raw = flags & R3D_NORMALS_RAW;
    if (d_tn && nt) k_tm_triangle_normals<<<r3d_blocks(nt), 256, 0, st>>>(d_pos, d_tri, nt, raw, d_tn);
    if (d_vn) k_tm_vertex_normals<<<r3d_blocks(nv), 256, 0, st>>>(d_pos, d_tri, T.inc_off, T.inc, (int)nv, raw, d_vn);
    R3D_HIP(ctx, hipGetLastError());
    return R3D_OK;
}

// ---- compaction ---------------------------------------------------------------------------------------------------------------------
struct TmCompact {
    int64_t nv, nt;
    r3d_mesh_in in;
    const uint8_t *vkeep, *tkeep;
    int flags;
    int64_t cap_v, cap_t;
    r3d_mesh_out out;
};
constexpr int TM_COMPACT_FLAGS = R3D_COMPACT_DROP_DEGENERATE | R3D_COMPACT_DROP_UNREFERENCED | R3D_COMPACT_DROP_NON_FINITE;

int tm_compact_args_ok(r3d_ctx *ctx, const TmCompact &m, const void *out_nv, const void *out_nt) {
    if (int rc = r3d_mesh_sizes_ok(ctx, "trimesh_compact", m.nv, m.nt)) return rc;
    if (m.flags & ~TM_COMPACT_FLAGS) return r3d_fail(ctx, R3D_E_BADARG, "trimesh_compact: unknown flags %d", m.flags);
    if (!out_nv || !out_nt || m.cap_v < 0 || m.cap_t < 0 || (m.nv > 0 && !m.in.pos) || (m.nt > 0 && !m.in.tri) ||
        (m.cap_v > 0 && (!m.out.pos || (m.in.nrm && !m.out.nrm) || (m.in.col && !m.out.col))) || (m.cap_t > 0 && !m.out.tri))
        return r3d_fail(ctx, R3D_E_BADARG, "trimesh_compact: a missing array or a negative capacity");
    return R3D_OK;
}

// device arrays in; the counts always; rows into the device outputs only when both capacities suffice.  *wrote: rows were written.
int tm_compact(r3d_ctx *ctx, DevArena &ar, const TmCompact &m, int64_t *out_nv, int64_t *out_nt, bool *wrote) {
    hipStream_t st = ctx->stream;
    *out_nv = *out_nt = 0;
    *wrote = false;
    if (int rc = r3d_mesh_empty_ok(ctx, "trimesh_compact", m.nv, m.nt)) return rc;
    if (m.nv == 0) return R3D_OK;
    const int nv = (int)m.nv;
    const int64_t nt = m.nt;
    int *gone = (int *)ar.get((size_t)nv * 4);
    int *ref = (int *)ar.get((size_t)nv * 4);
    int *vkeep = (int *)ar.get((size_t)(nv + 1) * 4), *vmap = (int *)ar.get((size_t)(nv + 1) * 4);
    int *tkeep = (int *)ar.get((size_t)(nt + 1) * 4), *tmap = (int *)ar.get((size_t)(nt + 1) * 4);
    TmHdr *hdr = (TmHdr *)ar.get(sizeof(TmHdr));
    if (ar.rc) return ar.rc;
    R3D_HIP(ctx, hipMemsetAsync(ref, 0, (size_t)nv * 4, st));
    R3D_HIP(ctx, hipMemsetAsync(vkeep + nv, 0, 4, st));
    R3D_HIP(ctx, hipMemsetAsync(tkeep + nt, 0, 4, st));
    R3D_HIP(ctx, hipMemsetAsync(hdr, 0, sizeof(TmHdr), st));
    k_tm_vertex_gone<<<r3d_blocks(nv), 256, 0, st>>>(m.in.pos, m.vkeep, nv, m.flags & R3D_COMPACT_DROP_NON_FINITE, gone);
    if (nt) k_tm_triangle_keep<<<r3d_blocks(nt), 256, 0, st>>>(m.in.tri, m.tkeep, nt, nv, m.flags & R3D_COMPACT_DROP_DEGENERATE, gone, tkeep, ref, hdr);
    k_tm_vertex_keep<<<r3d_blocks(nv), 256, 0, st>>>(gone, ref, nv, m.flags & R3D_COMPACT_DROP_UNREFERENCED, vkeep);
    R3D_HIP(ctx, hipGetLastError());
    int rc;
    if ((rc = r3d_exclusive_scan_i32(ctx, ar, vkeep, vmap, (int64_t)nv + 1)) || (rc = r3d_exclusive_scan_i32(ctx, ar, tkeep, tmap, nt + 1))) return rc;
    TmHdr h = {};
    int kept_v = 0, kept_t = 0;
    if ((rc = r3d_read_back(ctx, {{&h, hdr, sizeof(TmHdr)}, {&kept_v, vmap + nv, 4}, {&kept_t, tmap + nt, 4}}))) return rc;
    if (h.bad_index) return r3d_fail(ctx, R3D_E_BADARG, "trimesh_compact: a triangle index outside [0, %d)", nv);
    *out_nv = kept_v;
    *out_nt = kept_t;
    if (m.cap_v == 0 && m.cap_t == 0) return R3D_OK;
    if ((rc = r3d_fits2(ctx, "trimesh_compact", "vertices", kept_v, "triangles", kept_t, m.cap_v, m.cap_t))) return rc;
    if (kept_v) {
        k_tm_scatter_rows<<<r3d_blocks(nv), 256, 0, st>>>(vkeep, vmap, nv, m.in.pos, m.out.pos);
        if (m.in.nrm) k_tm_scatter_rows<<<r3d_blocks(nv), 256, 0, st>>>(vkeep, vmap, nv, m.in.nrm, m.out.nrm);
        if (m.in.col) k_tm_scatter_rows<<<r3d_blocks(nv), 256, 0, st>>>(vkeep, vmap, nv, m.in.col, m.out.col);
    }
    if (kept_t) k_tm_scatter_triangles<<<r3d_blocks(nt), 256, 0, st>>>(tkeep, tmap, vmap, m.in.tri, nt, m.out.tri);
    R3D_HIP(ctx, hipGetLastError());
    *wrote = true;
    return R3D_OK;
}

}  // namespace

extern "C" {

int r3d_trimesh_incidence(r3d_ctx *ctx, int64_t nv, int64_t nt, const int32_t *triangles, int64_t cap, int32_t *offsets, int32_t *corners, int64_t *out_n) {
    R3D_ROCTX_RANGE("r3d_trimesh_incidence");
    if (!ctx) return R3D_E_BADARG;
    return tm_lists(ctx, "trimesh_incidence", false, nv, nt, triangles, cap, offsets, corners, out_n);
}

int r3d_trimesh_adjacency(r3d_ctx *ctx, int64_t nv, int64_t nt, const int32_t *triangles, int64_t cap, int32_t *offsets, int32_t *neighbours, int64_t *out_n) {
    R3D_ROCTX_RANGE("r3d_trimesh_adjacency");
    if (!ctx) return R3D_E_BADARG;
    return tm_lists(ctx, "trimesh_adjacency", true, nv, nt, triangles, cap, offsets, neighbours, out_n);
}

int r3d_trimesh_smooth(r3d_ctx *ctx, int64_t nv, int64_t nt, const double *vertices, const double *normals, const double *colors, const int32_t *triangles,
                       int32_t kind, int32_t iterations, double lambda, double mu, int32_t scope, double *out_vertices, double *out_normals,
                       double *out_colors) {
    R3D_ROCTX_RANGE("r3d_trimesh_smooth");
    if (!ctx) return R3D_E_BADARG;
    if (int rc = tm_smooth_args_ok(ctx, nv, nt, vertices, normals, colors, triangles, kind, iterations, lambda, mu, scope, out_vertices, out_normals, out_colors))
        return rc;
    R3D_HIP(ctx, hipSetDevice(ctx->device));
    DevArena ar(ctx);
    TmSmooth m = {nv, nt, {}, kind, iterations, scope, lambda, mu, {}};
    int rc;
    if ((rc = r3d_mesh_upload(ctx, ar, {vertices, normals, colors, triangles}, nv, nt, &m.in))) return rc;
    r3d_mesh_outputs(ar, m.in, nv, nt, false, &m.out);
    if (ar.rc) return ar.rc;
    if ((rc = tm_smooth(ctx, ar, m))) return rc;
    if ((rc = r3d_mesh_download(ctx, {out_vertices, out_normals, out_colors, nullptr}, m.out, nv, 0))) return rc;
    R3D_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return R3D_OK;
}

int r3d_trimesh_smooth_dev(r3d_ctx *ctx, int64_t nv, int64_t nt, const double *d_vertices, const double *d_normals, const double *d_colors,
                           const int32_t *d_triangles, int32_t kind, int32_t iterations, double lambda, double mu, int32_t scope, double *d_out_vertices,
                           double *d_out_normals, double *d_out_colors) {
    R3D_ROCTX_RANGE("r3d_trimesh_smooth_dev");
    if (!ctx) return R3D_E_BADARG;
    if (int rc = tm_smooth_args_ok(ctx, nv, nt, d_vertices, d_normals, d_colors, d_triangles, kind, iterations, lambda, mu, scope, d_out_vertices, d_out_normals,
                                   d_out_colors))
        return rc;
    {
        const size_t rows = (size_t)nv * 24;
        const r3d_span out[] = {{d_out_vertices, rows}, {d_out_normals, d_normals ? rows : 0}, {d_out_colors, d_colors ? rows : 0}};
        const r3d_span in[] = {{d_vertices, rows}, {d_normals, rows}, {d_colors, rows}, {d_triangles, (size_t)nt * 12}};
        if (int rc = r3d_distinct(ctx, "trimesh_smooth_dev", out, 3, in, 4)) return rc;
    }
    R3D_HIP(ctx, hipSetDevice(ctx->device));
    DevArena ar(ctx);
    const TmSmooth m = {nv, nt, {d_vertices, d_normals, d_colors, d_triangles}, kind, iterations, scope, lambda, mu,
                        {d_out_vertices, d_out_normals, d_out_colors, nullptr}};
    if (int rc = tm_smooth(ctx, ar, m)) return rc;
    R3D_HIP(ctx, hipStreamSynchronize(ctx->stream));   // the steps read arena buffers the next call may hand out again
    return R3D_OK;
}

int r3d_trimesh_normals(r3d_ctx *ctx, int64_t nv, int64_t nt, const double *vertices, const int32_t *triangles, int32_t flags, double *triangle_normals,
                        double *vertex_normals) {
    R3D_ROCTX_RANGE("r3d_trimesh_normals");
    if (!ctx) return R3D_E_BADARG;
    if (int rc = tm_normals_args_ok(ctx, nv, nt, vertices, triangles, flags)) return rc;
    R3D_HIP(ctx, hipSetDevice(ctx->device));
    DevArena ar(ctx);
    r3d_mesh_in d;
    int rc;
    if ((rc = r3d_mesh_upload(ctx, ar, {vertices, nullptr, nullptr, triangles}, nv, nt, &d))) return rc;
    double *d_tn = triangle_normals ? (double *)ar.get((size_t)nt * 24) : nullptr;
    double *d_vn = vertex_normals ? (double *)ar.get((size_t)nv * 24) : nullptr;
    if (ar.rc) return ar.rc;
    if ((rc = tm_normals(ctx, ar, nv, nt, d.pos, d.tri, flags, d_tn, d_vn))) return rc;
    if ((rc = r3d_download(ctx, triangle_normals, d_tn, (size_t)nt * 3)) || (rc = r3d_download(ctx, vertex_normals, d_vn, (size_t)nv * 3))) return rc;
    R3D_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return R3D_OK;
}

int r3d_trimesh_normals_dev(r3d_ctx *ctx, int64_t nv, int64_t nt, const double *d_vertices, const int32_t *d_triangles, int32_t flags,
                            double *d_triangle_normals, double *d_vertex_normals) {
    R3D_ROCTX_RANGE("r3d_trimesh_normals_dev");
    if (!ctx) return R3D_E_BADARG;
    if (int rc = tm_normals_args_ok(ctx, nv, nt, d_vertices, d_triangles, flags)) return rc;
    {
        const r3d_span out[] = {{d_triangle_normals, (size_t)nt * 24}, {d_vertex_normals, (size_t)nv * 24}};
        const r3d_span in[] = {{d_vertices, (size_t)nv * 24}, {d_triangles, (size_t)nt * 12}};
        if (int rc = r3d_distinct(ctx, "trimesh_normals_dev", out, 2, in, 2)) return rc;
    }
    R3D_HIP(ctx, hipSetDevice(ctx->device));
    DevArena ar(ctx);
    if (int rc = tm_normals(ctx, ar, nv, nt, d_vertices, d_triangles, flags, d_triangle_normals, d_vertex_normals)) return rc;
    R3D_HIP(ctx, hipStreamSynchronize(ctx->stream));   // the vertex normals read the arena's incidence list
    return R3D_OK;
}

int r3d_trimesh_compact(r3d_ctx *ctx, int64_t nv, int64_t nt, const double *vertices, const double *normals, const double *colors, const int32_t *triangles,
                        const uint8_t *vertex_keep, const uint8_t *triangle_keep, int32_t flags, int64_t cap_vertices, int64_t cap_triangles,
                        double *out_vertices, double *out_normals, double *out_colors, int32_t *out_triangles, int64_t *out_nv, int64_t *out_nt) {
    R3D_ROCTX_RANGE("r3d_trimesh_compact");
    if (!ctx) return R3D_E_BADARG;
    const r3d_mesh_in h_in = {vertices, normals, colors, triangles};
    const r3d_mesh_out h_out = {out_vertices, out_normals, out_colors, out_triangles};
    TmCompact m = {nv, nt, h_in, vertex_keep, triangle_keep, flags, cap_vertices, cap_triangles, h_out};
    if (int rc = tm_compact_args_ok(ctx, m, out_nv, out_nt)) return rc;
    R3D_HIP(ctx, hipSetDevice(ctx->device));
    DevArena ar(ctx);
    int rc;
    if ((rc = r3d_mesh_upload(ctx, ar, h_in, nv, nt, &m.in)) || (rc = r3d_upload(ctx, ar, vertex_keep, (size_t)nv, &m.vkeep)) ||
        (rc = r3d_upload(ctx, ar, triangle_keep, (size_t)nt, &m.tkeep)))
        return rc;
    r3d_mesh_outputs(ar, m.in, nv, nt, true, &m.out);
    if (ar.rc) return ar.rc;
    bool wrote = false;
    if ((rc = tm_compact(ctx, ar, m, out_nv, out_nt, &wrote))) return rc;
    if (!wrote) return R3D_OK;
    if ((rc = r3d_mesh_download(ctx, h_out, m.out, *out_nv, *out_nt))) return rc;
    R3D_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return R3D_OK;
}

int r3d_trimesh_compact_dev(r3d_ctx *ctx, int64_t nv, int64_t nt, const double *d_vertices, const double *d_normals, const double *d_colors,
                            const int32_t *d_triangles, const uint8_t *d_vertex_keep, const uint8_t *d_triangle_keep, int32_t flags, int64_t cap_vertices,
                            int64_t cap_triangles, double *d_out_vertices, double *d_out_normals, double *d_out_colors, int32_t *d_out_triangles,
                            int64_t *out_nv, int64_t *out_nt) {
    R3D_ROCTX_RANGE("r3d_trimesh_compact_dev");
    if (!ctx) return R3D_E_BADARG;
    const TmCompact m = {nv, nt, {d_vertices, d_normals, d_colors, d_triangles}, d_vertex_keep, d_triangle_keep, flags, cap_vertices, cap_triangles,
                         {d_out_vertices, d_out_normals, d_out_colors, d_out_triangles}};
    if (int rc = tm_compact_args_ok(ctx, m, out_nv, out_nt)) return rc;
    {
        const size_t rows = (size_t)nv * 24, orows = (size_t)cap_vertices * 24;
        const r3d_span out[] = {{d_out_vertices, orows}, {d_out_normals, d_normals ? orows : 0}, {d_out_colors, d_colors ? orows : 0},
                                {d_out_triangles, (size_t)cap_triangles * 12}};
        const r3d_span in[] = {{d_vertices, rows}, {d_normals, rows}, {d_colors, rows}, {d_triangles, (size_t)nt * 12}, {d_vertex_keep, (size_t)nv},
                               {d_triangle_keep, (size_t)nt}};
        if (int rc = r3d_distinct(ctx, "trimesh_compact_dev", out, 4, in, 6)) return rc;
    }
    R3D_HIP(ctx, hipSetDevice(ctx->device));
    DevArena ar(ctx);
    bool wrote = false;
    if (int rc = tm_compact(ctx, ar, m, out_nv, out_nt, &wrote)) return rc;
    R3D_HIP(ctx, hipStreamSynchronize(ctx->stream));   // the scatters read arena buffers the next call may hand out again
    return R3D_OK;
}

}  // extern "C"
