// Mesh topology on the device ("Mesh topology"; C ABI: r3d_meshtopo_*): the edge table of a triangle mesh, its
// connected components with their triangle counts and areas, and the welds that remove duplicated vertices and triangles.
// tests/meshtopo_ref.py restates every result in numpy.
//
// Everything rests on one stable radix sort (cloud.hip: r3d_sort_pairs_u64).  Sides sorted by (min, max) put the sides of one edge
// side by side; vertices sorted by their coordinates' bit patterns and triangles sorted by their rotated index triple put duplicates
// side by side, the first occurrence in front because the sort is stable and the values start as the index.  Atomics hook union-find
// roots and count; the hooks always put the larger root under the smaller, so every component's root is its lowest triangle
// whatever the arrival order, and no arrival order reaches a result.  No kernel waits for another workgroup: every walk is capped
// and a trip over the cap raises an error word (R3D_E_INTERNAL).
#include "r3d_mesh.h"

#include <climits>

namespace {

typedef unsigned long long u64;

constexpr int MT_CHUNK = 256;   // terms per chunk of the component-area sum (chunks left to right, then chunk sums left to right)

struct MtHdr { int bad_index, walk_cap, n_long, pad; };
struct MtStats { int n_edges, boundary, non_manifold, degenerate; };

// ---- sides and the edge table -------------------------------------------------------------------------------------------------------
// one thread per side 3 t + c = (tri[t][c], tri[t][c + 1 mod 3]): key (min << b) | max.  An index outside [0, nv) raises the flag
// and the side gets key 0; nothing is addressed by an index here.
__global__ void __launch_bounds__(256) k_mt_sides(const int32_t *__restrict__ tri, int64_t n3, int nv, int b, u64 *__restrict__ key, MtHdr *__restrict__ hdr) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n3) return;
    const int64_t t = i / 3;
    const int c = (int)(i - 3 * t);
    int p = tri[i], q = tri[3 * t + (c == 2 ? 0 : c + 1)];
    if ((unsigned)p >= (unsigned)nv || (unsigned)q >= (unsigned)nv) { hdr->bad_index = 1; p = q = 0; }
    const int lo = p < q ? p : q, hi = p < q ? q : p;
    key[i] = ((u64)lo << b) | (u64)hi;
}

// head[i] = 1 where sorted entry i starts a run of equal keys; head[n] = 0 closes the array for the scan
__global__ void __launch_bounds__(256) k_mt_heads(const u64 *__restrict__ key, int64_t n, int *__restrict__ head) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i > n) return;
    head[i] = i < n && (i == 0 || key[i] != key[i - 1]);
}

// ex = exclusive scan of head: a head at i is edge ex[i]
__global__ void __launch_bounds__(256) k_mt_edge_rows(const u64 *__restrict__ key, const int *__restrict__ head, const int *__restrict__ ex, int64_t n, int b,
                                                      int *__restrict__ start, int32_t *__restrict__ edges) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n || !head[i]) return;
    const int e = ex[i];
    const u64 k = key[i];
    start[e] = (int)i;
    edges[2 * (int64_t)e] = (int32_t)(k >> b);
    edges[2 * (int64_t)e + 1] = (int32_t)(k & (((u64)1 << b) - 1));
}

// counts from the head positions; the statistics are counted per wave by ballot and added once per wave
__global__ void __launch_bounds__(256) k_mt_edge_counts(const int *__restrict__ start, const int *__restrict__ ex, int64_t n, const int32_t *__restrict__ edges,
                                                        int *__restrict__ counts, MtStats *__restrict__ st) {
    const int ne = ex[n];
    const int e = blockIdx.x * 256 + threadIdx.x;
    int c = 0;
    bool degenerate = false;
    if (e < ne) {
        c = (e + 1 < ne ? start[e + 1] : (int)n) - start[e];
        counts[e] = c;
        degenerate = edges[2 * (int64_t)e] == edges[2 * (int64_t)e + 1];
    }
    const int n1 = __popcll(__ballot(c == 1)), n3 = __popcll(__ballot(c > 2)), nd = __popcll(__ballot(degenerate));
    if ((threadIdx.x & 63) == 0) {
        if (n1) atomicAdd(&st->boundary, n1);
        if (n3) atomicAdd(&st->non_manifold, n3);
        if (nd) atomicAdd(&st->degenerate, nd);
        if (blockIdx.x == 0 && threadIdx.x == 0) st->n_edges = ne;
    }
}

// ---- components ---------------------------------------------------------------------------------------------------------------------
// gfx950: the eight XCDs have private L2s, so a plain load of a parent another workgroup hooked in this launch may be stale.  Every
// load of the forest inside the linking launch is a relaxed agent-scope atomic load, every change an atomic on the current value.
// A stale parent would still be an ancestor (a node only ever moves towards its root), so the walk stays correct either way.
__device__ __forceinline__ int mt_parent(const int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__global__ void __launch_bounds__(256) k_mt_iota(int *__restrict__ a, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) a[i] = (int)i;
}

// the root of x, halving the path on the way (a non-root's parent only ever decreases: atomicMin); -1 after more than `cap` steps
__device__ __forceinline__ int mt_find(int *parent, int x, int cap) {
    for (int s = 0; s <= cap; s++) {
        const int p = mt_parent(&parent[x]);
        if (p == x) return x;
        const int g = mt_parent(&parent[p]);
        if (g != p) atomicMin(&parent[x], g);
        x = g;
    }
    return -1;
}

// sorted sides i - 1 and i of one edge link their triangles: the larger root is hooked under the smaller by compare-and-swap on
// the root itself; a lost race means somebody else hooked it, and the walk goes on from there.  Never waits: every retry follows
// another thread's progress, and at most nt hooks can happen at all.
__global__ void __launch_bounds__(256) k_mt_link(const int *__restrict__ side, const int *__restrict__ head, int64_t n3, int nt, int *__restrict__ parent,
                                                 MtHdr *__restrict__ hdr) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < 1 || i >= n3 || head[i]) return;
    int a = side[i] / 3, b = side[i - 1] / 3;
    for (int s = 0; s <= nt; s++) {
        a = mt_find(parent, a, nt);
        b = mt_find(parent, b, nt);
        if (a < 0 || b < 0) break;
        if (a == b) return;
        const int hi = a > b ? a : b, lo = a > b ? b : a;
        if (atomicCAS(&parent[hi], hi, lo) == hi) return;
        a = hi;
        b = lo;
    }
    hdr->walk_cap = 1;
}

// a launch of its own: the forest no longer changes, plain loads, the root of every triangle into another array
__global__ void __launch_bounds__(256) k_mt_flatten(const int *__restrict__ parent, int nt, int *__restrict__ root, int *__restrict__ is_root,
                                                    MtHdr *__restrict__ hdr) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t > nt) return;
    if (t == nt) { is_root[t] = 0; return; }
    int x = t, s = 0;
    while (parent[x] != x && s <= nt) { x = parent[x]; s++; }
    if (parent[x] != x) hdr->walk_cap = 1;
    root[t] = x;
    is_root[t] = x == t;
}

// number[r] = how many roots lie below r: the components in ascending order of their lowest triangle
__global__ void __launch_bounds__(256) k_mt_labels(const int *__restrict__ root, const int *__restrict__ number, int nt, int32_t *__restrict__ label,
                                                   u64 *__restrict__ key) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= nt) return;
    const int l = number[root[t]];
    label[t] = l;
    key[t] = (u64)l;
}

// 0.5 |(p1 - p0) x (p2 - p0)| in the order written; runs after the host has seen bad_index == 0
__global__ void __launch_bounds__(256) k_mt_area(const double *__restrict__ pos, const int32_t *__restrict__ tri, int nt, double *__restrict__ area) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= nt) return;
    const int64_t i0 = 3 * (int64_t)tri[3 * (int64_t)t], i1 = 3 * (int64_t)tri[3 * (int64_t)t + 1], i2 = 3 * (int64_t)tri[3 * (int64_t)t + 2];
    const double a0 = pos[i1] - pos[i0], a1 = pos[i1 + 1] - pos[i0 + 1], a2 = pos[i1 + 2] - pos[i0 + 2];
    const double b0 = pos[i2] - pos[i0], b1 = pos[i2 + 1] - pos[i0 + 1], b2 = pos[i2 + 2] - pos[i0 + 2];
    const double n0 = a1 * b2 - a2 * b1, n1 = a2 * b0 - a0 * b2, n2 = a0 * b1 - a1 * b0;
    area[t] = 0.5 * sqrt((n0 * n0 + n1 * n1) + n2 * n2);
}

// the triangles sorted by label: a run's key is its label, so the head of run c is start[c]
__global__ void __launch_bounds__(256) k_mt_cluster_starts(const u64 *__restrict__ key, int nt, int *__restrict__ start) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nt) return;
    if (i == 0 || key[i] != key[i - 1]) start[key[i]] = i;
}

// one thread per component: the count, and the area of a list that is one chunk; longer lists go to the workgroup form
__global__ void __launch_bounds__(256) k_mt_cluster_short(const int *__restrict__ start, const int *__restrict__ order, const double *__restrict__ area, int ncl,
                                                          int nt, int64_t *__restrict__ count, double *__restrict__ sum, int *__restrict__ long_list,
                                                          MtHdr *__restrict__ hdr) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= ncl) return;
    const int b = start[c], n = (c + 1 < ncl ? start[c + 1] : nt) - b;
    count[c] = n;
    if (n > MT_CHUNK) { long_list[atomicAdd(&hdr->n_long, 1)] = c; return; }
    double s = 0.0;
    for (int j = 0; j < n; j++) s += area[order[b + j]];
    sum[c] = 0.0 + s;
}

// one workgroup per long list: thread k sums chunks k, k + 256, ... each from its front, then one thread adds the chunk sums from
// the front.  The shape depends on the list alone.  part is as long as the sorted list, and list c uses part[start[c] ...].
__global__ void __launch_bounds__(256) k_mt_cluster_long(const int *__restrict__ start, const int *__restrict__ order, const double *__restrict__ area, int ncl,
                                                         int nt, const int *__restrict__ long_list, const MtHdr *__restrict__ hdr, double *__restrict__ part,
                                                         double *__restrict__ sum) {
    if ((int)blockIdx.x >= hdr->n_long) return;
    const int c = long_list[blockIdx.x];
    const int b = start[c], n = (c + 1 < ncl ? start[c + 1] : nt) - b;
    const int chunks = (n + MT_CHUNK - 1) / MT_CHUNK;
    for (int k = threadIdx.x; k < chunks; k += 256) {
        const int j0 = k * MT_CHUNK, j1 = j0 + MT_CHUNK < n ? j0 + MT_CHUNK : n;
        double s = 0.0;
        for (int j = j0; j < j1; j++) s += area[order[b + j]];
        part[b + k] = s;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int k = 0; k < chunks; k++) s += part[b + k];
        sum[c] = s;
    }
}

// ---- welds --------------------------------------------------------------------------------------------------------------------------
// a coordinate's bit pattern with -0.0 folded to +0.0: equal doubles have equal keys (a NaN never equals: k_mt_vertex_heads)
__device__ __forceinline__ u64 mt_fold(double x) {
    const u64 u = (u64)__double_as_longlong(x);
    return u == 0x8000000000000000ull ? 0ull : u;
}

__global__ void __launch_bounds__(256) k_mt_vertex_keys(const double *__restrict__ pos, const int *__restrict__ perm, int nv, int axis, u64 *__restrict__ key) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nv) return;
    const int v = perm ? perm[i] : i;
    key[i] = mt_fold(pos[3 * (int64_t)v + axis]);
}

// neighbours in the sorted order are compared in full as doubles: -0.0 == +0.0, and a row with a NaN starts a run of its own
__global__ void __launch_bounds__(256) k_mt_vertex_heads(const double *__restrict__ pos, const int *__restrict__ perm, int nv, int *__restrict__ head) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i > nv) return;
    int h = 0;
    if (i < nv) {
        h = 1;
        if (i > 0) {
            const int64_t a = 3 * (int64_t)perm[i], b = 3 * (int64_t)perm[i - 1];
            h = !(pos[a] == pos[b] && pos[a + 1] == pos[b + 1] && pos[a + 2] == pos[b + 2]);
        }
    }
    head[i] = h;
}

__global__ void __launch_bounds__(256) k_mt_run_first(const int *__restrict__ perm, const int *__restrict__ head, const int *__restrict__ ex, int n,
                                                      int *__restrict__ run_first) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n && head[i]) run_first[ex[i]] = perm[i];
}

// first[v]: the lowest index of v's run (the sort is stable); keep[v] = v is that one; keep[n] = 0 closes the array for the scan
__global__ void __launch_bounds__(256) k_mt_first(const int *__restrict__ perm, const int *__restrict__ head, const int *__restrict__ ex,
                                                  const int *__restrict__ run_first, int n, int *__restrict__ first, int *__restrict__ keep) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i > n) return;
    if (i == n) { keep[n] = 0; return; }
    const int f = run_first[head[i] ? ex[i] : ex[i] - 1], v = perm[i];
    first[v] = f;
    keep[v] = f == v;
}

// the triangles through the vertex weld (first / vmap null: as they are).  An index outside [0, nv) raises the flag; the loads go
// to a clamped address.
__global__ void __launch_bounds__(256) k_mt_remap(const int32_t *__restrict__ tri, int64_t n3, int nv, const int *__restrict__ first, const int *__restrict__ vmap,
                                                  int32_t *__restrict__ out, MtHdr *__restrict__ hdr) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n3) return;
    int v = tri[i];
    if ((unsigned)v >= (unsigned)nv) { hdr->bad_index = 1; v = 0; }
    out[i] = first ? vmap[first[v]] : v;
}

// the rotation of (a, b, c) that is smallest in lexicographic order: the smallest index first, ties by what follows
__device__ __forceinline__ void mt_canon(const int32_t *__restrict__ tri, int64_t t, int &x, int &y, int &z) {
    const int a = tri[3 * t], b = tri[3 * t + 1], c = tri[3 * t + 2];
    x = a; y = b; z = c;
    if (b < x || (b == x && (c < y || (c == y && a < z)))) { x = b; y = c; z = a; }
    if (c < x || (c == x && (a < y || (a == y && b < z)))) { x = c; y = a; z = b; }
}

__global__ void __launch_bounds__(256) k_mt_triangle_keys(const int32_t *__restrict__ tri, const int *__restrict__ perm, int nt, int b, int low,
                                                          u64 *__restrict__ key) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nt) return;
    int x, y, z;
    mt_canon(tri, perm ? perm[i] : i, x, y, z);
    key[i] = low ? (u64)z : (((u64)x << b) | (u64)y);
}

__global__ void __launch_bounds__(256) k_mt_triangle_heads(const int32_t *__restrict__ tri, const int *__restrict__ perm, int nt, int *__restrict__ head) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i > nt) return;
    int h = 0;
    if (i < nt) {
        h = 1;
        if (i > 0) {
            int x0, y0, z0, x1, y1, z1;
            mt_canon(tri, perm[i], x0, y0, z0);
            mt_canon(tri, perm[i - 1], x1, y1, z1);
            h = !(x0 == x1 && y0 == y1 && z0 == z1);
        }
    }
    head[i] = h;
}

// keep / map null: every row stays where it is
__global__ void __launch_bounds__(256) k_mt_scatter_rows(const int *__restrict__ keep, const int *__restrict__ map, int nv, const double *__restrict__ src,
                                                         double *__restrict__ dst) {
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= nv || (keep && !keep[v])) return;
    const int64_t o = 3 * (int64_t)(map ? map[v] : v), i = 3 * (int64_t)v;
    dst[o] = src[i]; dst[o + 1] = src[i + 1]; dst[o + 2] = src[i + 2];
}

__global__ void __launch_bounds__(256) k_mt_scatter_triangles(const int *__restrict__ keep, const int *__restrict__ map, const int32_t *__restrict__ tri, int nt,
                                                              int32_t *__restrict__ out, int32_t *__restrict__ origin) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= nt || (keep && !keep[t])) return;
    const int64_t o = map ? map[t] : t;
    out[3 * o] = tri[3 * (int64_t)t]; out[3 * o + 1] = tri[3 * (int64_t)t + 1]; out[3 * o + 2] = tri[3 * (int64_t)t + 2];
    if (origin) origin[o] = t;
}

__global__ void __launch_bounds__(256) k_mt_vertex_map(const int *__restrict__ first, const int *__restrict__ vmap, int nv, int32_t *__restrict__ out) {
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v < nv) out[v] = first ? vmap[first[v]] : v;
}

// ====================================================================================================================== host side
inline int mt_bit_length(int64_t x) {
    int b = 0;
    while (x > 0) { b++; x >>= 1; }
    return b;
}

// the sides of nt > 0 triangles sorted by edge, with run heads and their scan; nothing read back yet
struct MtSides {
    const u64 *key = nullptr;    // [3 nt] sorted
    const int *side = nullptr;   // [3 nt] the side 3 t + c of each
    int *head = nullptr, *ex = nullptr;   // [3 nt + 1]
    MtHdr *hdr = nullptr;
    int b = 0;
};
int mt_sorted_sides(r3d_ctx *ctx, DevArena &ar, int nv, int64_t nt, const int32_t *d_tri, MtSides &S) {
    hipStream_t st = ctx->stream;
    const int64_t n3 = 3 * nt;
    S.b = mt_bit_length((int64_t)nv - 1);
    u64 *key = (u64 *)ar.get((size_t)n3 * 8);
    S.head = (int *)ar.get((size_t)(n3 + 1) * 4);
    S.ex = (int *)ar.get((size_t)(n3 + 1) * 4);
    S.hdr = (MtHdr *)ar.get(sizeof(MtHdr));
    if (ar.rc) return ar.rc;
    R3D_HIP(ctx, hipMemsetAsync(S.hdr, 0, sizeof(MtHdr), st));
    k_mt_sides<<<r3d_blocks(n3), 256, 0, st>>>(d_tri, n3, nv, S.b, key, S.hdr);
    R3D_HIP(ctx, hipGetLastError());
    const uint64_t *ks;
    if (int rc = r3d_sort_pairs_u64(ctx, ar, (const uint64_t *)key, nullptr, n3, 2 * S.b, &ks, &S.side)) return rc;
    S.key = (const u64 *)ks;
    k_mt_heads<<<r3d_blocks(n3 + 1), 256, 0, st>>>(S.key, n3, S.head);
    R3D_HIP(ctx, hipGetLastError());
    return r3d_exclusive_scan_i32(ctx, ar, S.head, S.ex, n3 + 1);
}

// ---- components: device arrays in and out.  d_labels [nt]; d_count / d_area [cap] are written when 0 < cap and the clusters fit.
int mt_components(r3d_ctx *ctx, DevArena &ar, const char *who, int64_t nv64, int64_t nt64, const double *d_pos, const int32_t *d_tri, int64_t cap,
                  int32_t *d_labels, int64_t *d_count, double *d_area, int64_t *out_ncl) {
    hipStream_t st = ctx->stream;
    *out_ncl = 0;
    if (nt64 == 0) return R3D_OK;
    if (int rc = r3d_mesh_empty_ok(ctx, who, nv64, nt64)) return rc;
    const int nv = (int)nv64, nt = (int)nt64;
    const int64_t n3 = 3 * nt64;
    MtSides S;
    if (int rc = mt_sorted_sides(ctx, ar, nv, nt, d_tri, S)) return rc;
    int *parent = (int *)ar.get((size_t)nt * 4), *root = (int *)ar.get((size_t)nt * 4);
    int *is_root = (int *)ar.get((size_t)(nt + 1) * 4), *number = (int *)ar.get((size_t)(nt + 1) * 4);
    int32_t *label = (int32_t *)ar.get((size_t)nt * 4);
    u64 *lkey = (u64 *)ar.get((size_t)nt * 8);
    if (ar.rc) return ar.rc;
    MtHdr h = {};
    if (int rc = r3d_read_back(ctx, {{&h, S.hdr, sizeof(MtHdr)}})) return rc;
    if (h.bad_index) return r3d_fail(ctx, R3D_E_BADARG, "%s: a triangle index outside [0, %d)", who, nv);
    k_mt_iota<<<r3d_blocks(nt), 256, 0, st>>>(parent, nt);
    k_mt_link<<<r3d_blocks(n3), 256, 0, st>>>(S.side, S.head, n3, nt, parent, S.hdr);
    k_mt_flatten<<<r3d_blocks(nt + 1), 256, 0, st>>>(parent, nt, root, is_root, S.hdr);
    R3D_HIP(ctx, hipGetLastError());
    if (int rc = r3d_exclusive_scan_i32(ctx, ar, is_root, number, (int64_t)nt + 1)) return rc;
    k_mt_labels<<<r3d_blocks(nt), 256, 0, st>>>(root, number, nt, label, lkey);
    R3D_HIP(ctx, hipGetLastError());
    int ncl = 0;
    if (int rc = r3d_read_back(ctx, {{&h, S.hdr, sizeof(MtHdr)}, {&ncl, number + nt, 4}})) return rc;
    if (h.walk_cap) return r3d_fail(ctx, R3D_E_INTERNAL, "%s: a union-find walk passed its cap of %d steps", who, nt);
    *out_ncl = ncl;
    if (cap > 0) {
        if (int rc = r3d_fits(ctx, who, "clusters", ncl, cap)) return rc;
        double *area = (double *)ar.get((size_t)nt * 8), *part = (double *)ar.get((size_t)nt * 8);
        int *start = (int *)ar.get((size_t)ncl * 4), *long_list = (int *)ar.get((size_t)(nt / MT_CHUNK + 1) * 4);
        if (ar.rc) return ar.rc;
        k_mt_area<<<r3d_blocks(nt), 256, 0, st>>>(d_pos, d_tri, nt, area);
        R3D_HIP(ctx, hipGetLastError());
        const uint64_t *ks;
        const int *order;
        if (int rc = r3d_sort_pairs_u64(ctx, ar, (const uint64_t *)lkey, nullptr, nt, mt_bit_length((int64_t)ncl - 1), &ks, &order)) return rc;
        k_mt_cluster_starts<<<r3d_blocks(nt), 256, 0, st>>>((const u64 *)ks, nt, start);
        k_mt_cluster_short<<<r3d_blocks(ncl), 256, 0, st>>>(start, order, area, ncl, nt, d_count, d_area, long_list, S.hdr);
        k_mt_cluster_long<<<(unsigned)(nt / MT_CHUNK + 1), 256, 0, st>>>(start, order, area, ncl, nt, long_list, S.hdr, part, d_area);
        R3D_HIP(ctx, hipGetLastError());
    }
    R3D_HIP(ctx, hipMemcpyAsync(d_labels, label, (size_t)nt * 4, hipMemcpyDeviceToDevice, st));
    return R3D_OK;
}

int mt_components_args_ok(r3d_ctx *ctx, const char *who, int64_t nv, int64_t nt, const void *vertices, const void *triangles, int64_t cap, const void *labels,
                          const void *counts, const void *areas, const void *out_n) {
    if (int rc = r3d_mesh_sizes_ok(ctx, who, nv, nt)) return rc;
    if (!out_n || cap < 0 || (nt > 0 && (!triangles || !labels)) || (cap > 0 && (!counts || !areas || (nv > 0 && !vertices))))
        return r3d_fail(ctx, R3D_E_BADARG, "%s: a missing array or a negative capacity", who);
    return R3D_OK;
}

// ---- welds --------------------------------------------------------------------------------------------------------------------------
// from a sorted order and its run heads: first[], keep[] and the scanned map[] (n + 1 entries, map[n] = rows kept)
int mt_group(r3d_ctx *ctx, DevArena &ar, int n, const int *perm, int *head, int **first, int **keep, int **map) {
    int *ex = (int *)ar.get((size_t)(n + 1) * 4), *run_first = (int *)ar.get((size_t)n * 4);
    *first = (int *)ar.get((size_t)n * 4);
    *keep = (int *)ar.get((size_t)(n + 1) * 4);
    *map = (int *)ar.get((size_t)(n + 1) * 4);
    if (ar.rc) return ar.rc;
    if (int rc = r3d_exclusive_scan_i32(ctx, ar, head, ex, (int64_t)n + 1)) return rc;
    k_mt_run_first<<<r3d_blocks(n), 256, 0, ctx->stream>>>(perm, head, ex, n, run_first);
    k_mt_first<<<r3d_blocks(n + 1), 256, 0, ctx->stream>>>(perm, head, ex, run_first, n, *first, *keep);
    R3D_HIP(ctx, hipGetLastError());
    return r3d_exclusive_scan_i32(ctx, ar, *keep, *map, (int64_t)n + 1);
}

struct MtDedup {
    int64_t nv, nt;
    r3d_mesh_in in;
    int flags;
    int64_t cap_v, cap_t;
    r3d_mesh_out out;
    int32_t *vertex_map, *triangle_origin;
};
constexpr int MT_DEDUP_FLAGS = R3D_DEDUP_VERTICES | R3D_DEDUP_TRIANGLES;

int mt_dedup_args_ok(r3d_ctx *ctx, const char *who, const MtDedup &m, const void *out_nv, const void *out_nt) {
    if (int rc = r3d_mesh_sizes_ok(ctx, who, m.nv, m.nt)) return rc;
    if (m.flags & ~MT_DEDUP_FLAGS) return r3d_fail(ctx, R3D_E_BADARG, "%s: unknown flags %d", who, m.flags);
    if (!out_nv || !out_nt || m.cap_v < 0 || m.cap_t < 0 || (m.nv > 0 && !m.in.pos) || (m.nt > 0 && !m.in.tri) ||
        (m.cap_v > 0 && (!m.out.pos || (m.in.nrm && !m.out.nrm) || (m.in.col && !m.out.col))) || (m.cap_t > 0 && !m.out.tri))
        return r3d_fail(ctx, R3D_E_BADARG, "%s: a missing array or a negative capacity", who);
    return R3D_OK;
}

// device arrays in; the counts always; rows into the device outputs only when both capacities suffice.  *wrote: rows were written.
int mt_dedup(r3d_ctx *ctx, DevArena &ar, const char *who, const MtDedup &m, int64_t *out_nv, int64_t *out_nt, bool *wrote) {
    hipStream_t st = ctx->stream;
    *out_nv = *out_nt = 0;
    *wrote = false;
    if (int rc = r3d_mesh_empty_ok(ctx, who, m.nv, m.nt)) return rc;
    if (m.nv == 0) return R3D_OK;
    const int nv = (int)m.nv, nt = (int)m.nt;
    const int64_t n3 = 3 * m.nt;
    const int b = mt_bit_length((int64_t)nv - 1);
    MtHdr *hdr = (MtHdr *)ar.get(sizeof(MtHdr));
    if (ar.rc) return ar.rc;
    R3D_HIP(ctx, hipMemsetAsync(hdr, 0, sizeof(MtHdr), st));
    int *vfirst = nullptr, *vkeep = nullptr, *vmap = nullptr;
    if (m.flags & R3D_DEDUP_VERTICES) {
        // x, then y, then z decide: three chained sorts, z first, each key gathered through the order so far
        u64 *key = (u64 *)ar.get((size_t)nv * 8);
        int *head = (int *)ar.get((size_t)(nv + 1) * 4);
        if (ar.rc) return ar.rc;
        const int *perm = nullptr;
        for (int axis = 2; axis >= 0; axis--) {
            k_mt_vertex_keys<<<r3d_blocks(nv), 256, 0, st>>>(m.in.pos, perm, nv, axis, key);
            R3D_HIP(ctx, hipGetLastError());
            const uint64_t *ks;
            if (int rc = r3d_sort_pairs_u64(ctx, ar, (const uint64_t *)key, perm, nv, 64, &ks, &perm)) return rc;
        }
        k_mt_vertex_heads<<<r3d_blocks(nv + 1), 256, 0, st>>>(m.in.pos, perm, nv, head);
        R3D_HIP(ctx, hipGetLastError());
        if (int rc = mt_group(ctx, ar, nv, perm, head, &vfirst, &vkeep, &vmap)) return rc;
    }
    int32_t *tri2 = (int32_t *)ar.get((size_t)n3 * 4);
    if (ar.rc) return ar.rc;
    if (nt) k_mt_remap<<<r3d_blocks(n3), 256, 0, st>>>(m.in.tri, n3, nv, vfirst, vmap, tri2, hdr);
    R3D_HIP(ctx, hipGetLastError());
    int *tfirst = nullptr, *tkeep = nullptr, *tmap = nullptr;
    if ((m.flags & R3D_DEDUP_TRIANGLES) && nt) {
        // (a, b) then c decide: c first, then (a << b) | b gathered through that order
        u64 *key = (u64 *)ar.get((size_t)nt * 8);
        int *head = (int *)ar.get((size_t)(nt + 1) * 4);
        if (ar.rc) return ar.rc;
        const uint64_t *ks;
        const int *perm = nullptr;
        k_mt_triangle_keys<<<r3d_blocks(nt), 256, 0, st>>>(tri2, nullptr, nt, b, 1, key);
        R3D_HIP(ctx, hipGetLastError());
        if (int rc = r3d_sort_pairs_u64(ctx, ar, (const uint64_t *)key, nullptr, nt, b, &ks, &perm)) return rc;
        k_mt_triangle_keys<<<r3d_blocks(nt), 256, 0, st>>>(tri2, perm, nt, b, 0, key);
        R3D_HIP(ctx, hipGetLastError());
        if (int rc = r3d_sort_pairs_u64(ctx, ar, (const uint64_t *)key, perm, nt, 2 * b, &ks, &perm)) return rc;
        k_mt_triangle_heads<<<r3d_blocks(nt + 1), 256, 0, st>>>(tri2, perm, nt, head);
        R3D_HIP(ctx, hipGetLastError());
        if (int rc = mt_group(ctx, ar, nt, perm, head, &tfirst, &tkeep, &tmap)) return rc;
    }
    MtHdr h = {};
    int kept_v = nv, kept_t = nt;
    if (int rc = r3d_read_back(ctx, {{&h, hdr, sizeof(MtHdr)}, {&kept_v, vmap ? vmap + nv : nullptr, 4}, {&kept_t, tmap ? tmap + nt : nullptr, 4}})) return rc;
    if (h.bad_index) return r3d_fail(ctx, R3D_E_BADARG, "%s: a triangle index outside [0, %d)", who, nv);
    *out_nv = kept_v;
    *out_nt = kept_t;
    if (m.cap_v == 0 && m.cap_t == 0) return R3D_OK;
    if (int rc = r3d_fits2(ctx, who, "vertices", kept_v, "triangles", kept_t, m.cap_v, m.cap_t)) return rc;
    k_mt_scatter_rows<<<r3d_blocks(nv), 256, 0, st>>>(vkeep, vmap, nv, m.in.pos, m.out.pos);
    if (m.in.nrm) k_mt_scatter_rows<<<r3d_blocks(nv), 256, 0, st>>>(vkeep, vmap, nv, m.in.nrm, m.out.nrm);
    if (m.in.col) k_mt_scatter_rows<<<r3d_blocks(nv), 256, 0, st>>>(vkeep, vmap, nv, m.in.col, m.out.col);
    if (m.vertex_map) k_mt_vertex_map<<<r3d_blocks(nv), 256, 0, st>>>(vfirst, vmap, nv, m.vertex_map);
    if (nt) k_mt_scatter_triangles<<<r3d_blocks(nt), 256, 0, st>>>(tkeep, tmap, tri2, nt, m.out.tri, m.triangle_origin);
    R3D_HIP(ctx, hipGetLastError());
    *wrote = true;
    return R3D_OK;
}

}  // namespace

extern "C" {

int r3d_meshtopo_edges(r3d_ctx *ctx, int64_t nv, int64_t nt, const int32_t *triangles, int64_t cap, int32_t *edges, int32_t *counts, int64_t *stats,
                       int64_t *out_n) {
    R3D_ROCTX_RANGE("r3d_meshtopo_edges");
    if (!ctx) return R3D_E_BADARG;
    const char *who = "meshtopo_edges";
    if (int rc = r3d_mesh_sizes_ok(ctx, who, nv, nt)) return rc;
    if (!out_n || cap < 0 || (nt > 0 && !triangles) || (cap > 0 && (!edges || !counts)))
        return r3d_fail(ctx, R3D_E_BADARG, "%s: a missing array or a negative capacity", who);
    *out_n = 0;
    if (stats) stats[0] = stats[1] = stats[2] = stats[3] = 0;
    R3D_HIP(ctx, hipSetDevice(ctx->device));
    if (nt == 0) return R3D_OK;
    if (int rc = r3d_mesh_empty_ok(ctx, who, nv, nt)) return rc;
    DevArena ar(ctx);
    hipStream_t st = ctx->stream;
    const int64_t n3 = 3 * nt;
    const int32_t *d_tri;
    if (int rc = r3d_upload(ctx, ar, triangles, (size_t)n3, &d_tri)) return rc;
    MtSides S;
    if (int rc = mt_sorted_sides(ctx, ar, (int)nv, nt, d_tri, S)) return rc;
    int *start = (int *)ar.get((size_t)n3 * 4), *d_counts = (int *)ar.get((size_t)n3 * 4);
    int32_t *d_edges = (int32_t *)ar.get((size_t)n3 * 8);
    MtStats *d_stats = (MtStats *)ar.get(sizeof(MtStats));
    if (ar.rc) return ar.rc;
    MtHdr h = {};
    int ne = 0;
    if (int rc = r3d_read_back(ctx, {{&h, S.hdr, sizeof(MtHdr)}, {&ne, S.ex + n3, 4}})) return rc;
    if (h.bad_index) return r3d_fail(ctx, R3D_E_BADARG, "%s: a triangle index outside [0, %d)", who, (int)nv);
    R3D_HIP(ctx, hipMemsetAsync(d_stats, 0, sizeof(MtStats), st));
    k_mt_edge_rows<<<r3d_blocks(n3), 256, 0, st>>>(S.key, S.head, S.ex, n3, S.b, start, d_edges);
    k_mt_edge_counts<<<r3d_blocks(ne), 256, 0, st>>>(start, S.ex, n3, d_edges, d_counts, d_stats);
    R3D_HIP(ctx, hipGetLastError());
    MtStats hs = {};
    if (int rc = r3d_read_back(ctx, {{&hs, d_stats, sizeof(MtStats)}})) return rc;
    *out_n = ne;
    if (stats) { stats[0] = hs.n_edges; stats[1] = hs.boundary; stats[2] = hs.non_manifold; stats[3] = hs.degenerate; }
    if (cap == 0) return R3D_OK;
    if (int rc = r3d_fits(ctx, who, "edges", ne, cap)) return rc;
    int rc;
    if ((rc = r3d_download(ctx, edges, (const int32_t *)d_edges, (size_t)ne * 2)) || (rc = r3d_download(ctx, counts, (const int32_t *)d_counts, (size_t)ne))) return rc;
    R3D_HIP(ctx, hipStreamSynchronize(st));
    return R3D_OK;
}

int r3d_meshtopo_components(r3d_ctx *ctx, int64_t nv, int64_t nt, const double *vertices, const int32_t *triangles, int64_t cap_clusters,
                            int32_t *triangle_clusters, int64_t *cluster_n_triangles, double *cluster_area, int64_t *out_n_clusters) {
    R3D_ROCTX_RANGE("r3d_meshtopo_components");
    if (!ctx) return R3D_E_BADARG;
    const char *who = "meshtopo_components";
    if (int rc = mt_components_args_ok(ctx, who, nv, nt, vertices, triangles, cap_clusters, triangle_clusters, cluster_n_triangles, cluster_area, out_n_clusters))
        return rc;
    R3D_HIP(ctx, hipSetDevice(ctx->device));
    DevArena ar(ctx);
    r3d_mesh_in d;   // the areas alone read the vertices
    int rc;
    if ((rc = r3d_mesh_upload(ctx, ar, {cap_clusters > 0 ? vertices : nullptr, nullptr, nullptr, triangles}, nv, nt, &d))) return rc;
    int32_t *d_labels = (int32_t *)ar.get((size_t)nt * 4);
    int64_t *d_count = cap_clusters > 0 ? (int64_t *)ar.get((size_t)cap_clusters * 8) : nullptr;
    double *d_area = cap_clusters > 0 ? (double *)ar.get((size_t)cap_clusters * 8) : nullptr;
    if (ar.rc) return ar.rc;
    if ((rc = mt_components(ctx, ar, who, nv, nt, d.pos, d.tri, cap_clusters, d_labels, d_count, d_area, out_n_clusters))) return rc;
    const size_t ncl = cap_clusters > 0 ? (size_t)*out_n_clusters : 0;
    if ((rc = r3d_download(ctx, triangle_clusters, (const int32_t *)d_labels, (size_t)nt)) ||
        (rc = r3d_download(ctx, cluster_n_triangles, (const int64_t *)d_count, ncl)) || (rc = r3d_download(ctx, cluster_area, (const double *)d_area, ncl)))
        return rc;
    R3D_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return R3D_OK;
}

int r3d_meshtopo_components_dev(r3d_ctx *ctx, int64_t nv, int64_t nt, const double *d_vertices, const int32_t *d_triangles, int64_t cap_clusters,
                                int32_t *d_triangle_clusters, int64_t *d_cluster_n_triangles, double *d_cluster_area, int64_t *out_n_clusters) {
    R3D_ROCTX_RANGE("r3d_meshtopo_components_dev");
    if (!ctx) return R3D_E_BADARG;
    const char *who = "meshtopo_components_dev";
    if (int rc = mt_components_args_ok(ctx, who, nv, nt, d_vertices, d_triangles, cap_clusters, d_triangle_clusters, d_cluster_n_triangles, d_cluster_area,
                                       out_n_clusters))
        return rc;
    {
        const r3d_span out[] = {{d_triangle_clusters, (size_t)nt * 4}, {d_cluster_n_triangles, (size_t)cap_clusters * 8}, {d_cluster_area, (size_t)cap_clusters * 8}};
        const r3d_span in[] = {{d_vertices, (size_t)nv * 24}, {d_triangles, (size_t)nt * 12}};
        if (int rc = r3d_distinct(ctx, who, out, 3, in, 2)) return rc;
    }
    R3D_HIP(ctx, hipSetDevice(ctx->device));
    DevArena ar(ctx);
    if (int rc = mt_components(ctx, ar, who, nv, nt, d_vertices, d_triangles, cap_clusters, d_triangle_clusters, d_cluster_n_triangles, d_cluster_area,
                               out_n_clusters))
        return rc;
    R3D_HIP(ctx, hipStreamSynchronize(ctx->stream));   // the last kernels read arena buffers the next call may hand out again
    return R3D_OK;
}

int r3d_meshtopo_dedup(r3d_ctx *ctx, int64_t nv, int64_t nt, const double *vertices, const double *normals, const double *colors, const int32_t *triangles,
                       int32_t flags, int64_t cap_vertices, int64_t cap_triangles, double *out_vertices, double *out_normals, double *out_colors,
                       int32_t *out_triangles, int32_t *vertex_map, int32_t *triangle_origin, int64_t *out_nv, int64_t *out_nt) {
    R3D_ROCTX_RANGE("r3d_meshtopo_dedup");
    if (!ctx) return R3D_E_BADARG;
    const char *who = "meshtopo_dedup";
    const r3d_mesh_in h_in = {vertices, normals, colors, triangles};
    const r3d_mesh_out h_out = {out_vertices, out_normals, out_colors, out_triangles};
    MtDedup m = {nv, nt, h_in, flags, cap_vertices, cap_triangles, h_out, vertex_map, triangle_origin};
    if (int rc = mt_dedup_args_ok(ctx, who, m, out_nv, out_nt)) return rc;
    R3D_HIP(ctx, hipSetDevice(ctx->device));
    DevArena ar(ctx);
    int rc;
    if ((rc = r3d_mesh_upload(ctx, ar, h_in, nv, nt, &m.in))) return rc;
    r3d_mesh_outputs(ar, m.in, nv, nt, true, &m.out);
    m.vertex_map = vertex_map ? (int32_t *)ar.get((size_t)nv * 4) : nullptr;
    m.triangle_origin = triangle_origin ? (int32_t *)ar.get((size_t)nt * 4) : nullptr;
    if (ar.rc) return ar.rc;
    bool wrote = false;
    if ((rc = mt_dedup(ctx, ar, who, m, out_nv, out_nt, &wrote))) return rc;
    if (!wrote) return R3D_OK;
    if ((rc = r3d_mesh_download(ctx, h_out, m.out, *out_nv, *out_nt)) || (rc = r3d_download(ctx, vertex_map, (const int32_t *)m.vertex_map, (size_t)nv)) ||
        (rc = r3d_download(ctx, triangle_origin, (const int32_t *)m.triangle_origin, (size_t)*out_nt)))
        return rc;
    R3D_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return R3D_OK;
}

int r3d_meshtopo_dedup_dev(r3d_ctx *ctx, int64_t nv, int64_t nt, const double *d_vertices, const double *d_normals, const double *d_colors,
                           const int32_t *d_triangles, int32_t flags, int64_t cap_vertices, int64_t cap_triangles, double *d_out_vertices,
                           double *d_out_normals, double *d_out_colors, int32_t *d_out_triangles, int32_t *d_vertex_map, int32_t *d_triangle_origin,
                           int64_t *out_nv, int64_t *out_nt) {
    R3D_ROCTX_RANGE("r3d_meshtopo_dedup_dev");
    if (!ctx) return R3D_E_BADARG;
    const char *who = "meshtopo_dedup_dev";
    const MtDedup m = {nv, nt, {d_vertices, d_normals, d_colors, d_triangles}, flags, cap_vertices, cap_triangles,
                       {d_out_vertices, d_out_normals, d_out_colors, d_out_triangles}, d_vertex_map, d_triangle_origin};
    if (int rc = mt_dedup_args_ok(ctx, who, m, out_nv, out_nt)) return rc;
    {
        const size_t rows = (size_t)nv * 24, orows = (size_t)cap_vertices * 24;
        const r3d_span out[] = {{d_out_vertices, orows}, {d_out_normals, d_normals ? orows : 0}, {d_out_colors, d_colors ? orows : 0},
                                {d_out_triangles, (size_t)cap_triangles * 12}, {d_vertex_map, (size_t)nv * 4}, {d_triangle_origin, (size_t)cap_triangles * 4}};
        const r3d_span in[] = {{d_vertices, rows}, {d_normals, rows}, {d_colors, rows}, {d_triangles, (size_t)nt * 12}};
        if (int rc = r3d_distinct(ctx, who, out, 6, in, 4)) return rc;
    }
    R3D_HIP(ctx, hipSetDevice(ctx->device));
    DevArena ar(ctx);
    bool wrote = false;
    if (int rc = mt_dedup(ctx, ar, who, m, out_nv, out_nt, &wrote)) return rc;
    R3D_HIP(ctx, hipStreamSynchronize(ctx->stream));   // the scatters read arena buffers the next call may hand out again
    return R3D_OK;
}

int r3d_debug_sort_pairs_u64(r3d_ctx *ctx, const uint64_t *keys, const int32_t *values, int64_t n, int32_t bits, uint64_t *out_keys, int32_t *out_values) {
    R3D_ROCTX_RANGE("r3d_debug_sort_pairs_u64");
    if (!ctx) return R3D_E_BADARG;
    if (n < 0 || (n > 0 && (!keys || !out_keys || !out_values))) return r3d_fail(ctx, R3D_E_BADARG, "debug_sort_pairs_u64: a missing array or a negative count");
    if (ctx->poisoned) return r3d_fail(ctx, R3D_E_HIP, "debug_sort_pairs_u64: context poisoned by an earlier timed-out call: destroy it");
    R3D_HIP(ctx, hipSetDevice(ctx->device));
    DevArena ar(ctx);
    const uint64_t *d_keys, *ks;
    const int32_t *d_vals, *vs;
    int rc;
    if ((rc = r3d_upload(ctx, ar, keys, (size_t)n, &d_keys)) || (rc = r3d_upload(ctx, ar, values, (size_t)n, &d_vals))) return rc;
    if ((rc = r3d_sort_pairs_u64(ctx, ar, d_keys, d_vals, n, bits, &ks, &vs))) return rc;
    if ((rc = r3d_download(ctx, out_keys, ks, (size_t)n)) || (rc = r3d_download(ctx, out_values, vs, (size_t)n))) return rc;
    R3D_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return R3D_OK;
}

}  // extern "C"
