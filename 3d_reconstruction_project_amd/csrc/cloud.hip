// cloud.hip -- point-cloud half of the hot path for gfx950: uniform-grid neighbour search, voxel down-sampling,
// hybrid / kNN PCA normals and the fused nearest-neighbour + Gauss-Newton reduction of ICP / point-to-plane / GICP.
//
// Replaces the Open3D (legacy, float64) calls the reference makes; semantics are those pinned in
// oracle/cloud_oracle.py (fixture-verified for voxel / normals / SOR, [recalled] Open3D for registration):
//   voxel_down_sample          pointcloud_alignment.py:22-23
//   estimate_normals(Hybrid)   pointcloud_alignment.py:27-28, test/GICP1.py:77, normal_estimation.py:20
//   registration_icp           pointcloud_alignment.py:35-39
//   registration_generalized_icp   test/GICP1.py:99-102     point-to-plane: test/check2.py:151-154
//   source.transform(T)        pointcloud_alignment.py:42
// All geometry is float64 like the legacy Open3D classes (MI355X runs fp64 vector math at half the fp32 rate,
// and these kernels are latency / LDS bound, not flop bound), which keeps voxel membership and neighbour sets
// identical to the oracle's instead of "within tolerance".

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>
#include <thread>
#include <vector>

#include "r3d_internal.h"

namespace {

struct GridView {
    double ox, oy, oz, cell, inv_cell;
    int nx, ny, nz;
    // Cell table, two levels.  cstart(c) = number of points whose cell index is below c = first sorted slot of cell c (x is the
    // fastest key digit, so cells adjacent in x hold ONE contiguous run of points).  The linear cell index is cut into LINES of 32
    // cells; l1[line] >= 0: no point in cells [32 line, 32 line + 36): all those cells share that cstart value;
    // l1[line] < 0: the line is materialised as l2[(-l1 - 1) * 36 + w], w = 0 .. 35 (the last four entries repeat the first four
    // cells of the next line, so a 16-byte read of four consecutive entries never leaves its line).  A surface occupies a few per
    // cent of a dense grid: at 1 M points the dense int table was 144 MB and most of a query's L2 misses; l1 is 4.5 MB, l2 ~15 MB.
    const int *l1, *l2;
    // ... or, when `dense` is set, the plain table dense[c] = cstart(c), c = 0 .. ncells + 4 (no dependent second load: what the
    // registration loop's search uses; its set-up pays three passes over the whole table instead)
    const int *dense;
    const double *pts;     // [n][3] points in cell-sorted order
    const int *idx;        // [n] sorted slot -> original index
    // optional packed copy for the registration loop's default search (nn_block_q10): one dword per sorted point = 10-bit offsets
    // inside its own cell (x | y << 12 | z << 22) and the low two bits of its cell x index (<< 10); n + 4 entries
    const unsigned *q10;
    int pool;              // 1 whenever q10 is set (k_icp_eval<*, SEARCH_Q10> tests it; why it stays a field: DESIGN.md section 7)
};

__device__ __forceinline__ int cell_coord(double v, double o, double inv) { return (int)floor((v - o) * inv); }

constexpr int CL_SHIFT = 5, CL_STRIDE = 36;
typedef int cs_int4 __attribute__((ext_vector_type(4), aligned(4)));   // dword-aligned 16-byte global load
// loads are issued unconditionally from a clamped address and selected afterwards (a branch around a load costs a wait per load)
__device__ __forceinline__ int cs1(const GridView &g, int64_t c) {
    if (g.dense) return g.dense[c];   // wave-uniform branch
    const int v = g.l1[c >> CL_SHIFT];
    const int e = g.l2[(int64_t)(v < 0 ? -v - 1 : 0) * CL_STRIDE + (int)(c & 31)];
    return v < 0 ? e : v;
}
// cstart of the four consecutive cells c .. c + 3
__device__ __forceinline__ cs_int4 cs4(const GridView &g, int64_t c) {
    if (g.dense) return *(const cs_int4 *)(g.dense + c);   // wave-uniform branch
    const int v = g.l1[c >> CL_SHIFT];
    const cs_int4 e = *(const cs_int4 *)(g.l2 + (int64_t)(v < 0 ? -v - 1 : 0) * CL_STRIDE + (int)(c & 31));
    cs_int4 r;
    r.x = v < 0 ? e.x : v; r.y = v < 0 ? e.y : v; r.z = v < 0 ? e.z : v; r.w = v < 0 ? e.w : v;
    return r;
}

// ------------------------------------------------------------------------------------------------ bbox
__global__ void __launch_bounds__(256) k_bbox_partial(const double *__restrict__ p, int64_t n, double *__restrict__ part) {
    double mn[3] = {1e300, 1e300, 1e300}, mx[3] = {-1e300, -1e300, -1e300};
    for (int64_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
        for (int a = 0; a < 3; a++) { double v = p[i * 3 + a]; mn[a] = fmin(mn[a], v); mx[a] = fmax(mx[a], v); }
    __shared__ double sm[6][256];
    for (int a = 0; a < 3; a++) { sm[a][threadIdx.x] = mn[a]; sm[3 + a][threadIdx.x] = mx[a]; }
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s)
            for (int a = 0; a < 3; a++) {
                sm[a][threadIdx.x] = fmin(sm[a][threadIdx.x], sm[a][threadIdx.x + s]);
                sm[3 + a][threadIdx.x] = fmax(sm[3 + a][threadIdx.x], sm[3 + a][threadIdx.x + s]);
            }
        __syncthreads();
    }
    if (threadIdx.x < 6) part[blockIdx.x * 6 + threadIdx.x] = sm[threadIdx.x][0];
}

// the same over a point count that is still on the device (n = *c0 + *c1: the last entries of a compaction's scan and flags):
// the bounding box is enqueued before the host knows how many points there are, and both come back in ONE read
__global__ void __launch_bounds__(256) k_bbox_partial_dn(const double *__restrict__ p, const int *__restrict__ c0, const int *__restrict__ c1,
                                                         double *__restrict__ part) {
    const int64_t n = (int64_t)*c0 + *c1;
    double mn[3] = {1e300, 1e300, 1e300}, mx[3] = {-1e300, -1e300, -1e300};
    for (int64_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
        for (int a = 0; a < 3; a++) { double v = p[i * 3 + a]; mn[a] = fmin(mn[a], v); mx[a] = fmax(mx[a], v); }
    __shared__ double sm[6][256];
    for (int a = 0; a < 3; a++) { sm[a][threadIdx.x] = mn[a]; sm[3 + a][threadIdx.x] = mx[a]; }
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s)
            for (int a = 0; a < 3; a++) {
                sm[a][threadIdx.x] = fmin(sm[a][threadIdx.x], sm[a][threadIdx.x + s]);
                sm[3 + a][threadIdx.x] = fmax(sm[3 + a][threadIdx.x], sm[3 + a][threadIdx.x + s]);
            }
        __syncthreads();
    }
    if (threadIdx.x < 6) part[blockIdx.x * 6 + threadIdx.x] = sm[threadIdx.x][0];
}

// second stage: one workgroup folds the per-workgroup boxes into one (6 doubles), so the host reads 48 bytes
__global__ void __launch_bounds__(256) k_bbox_final(const double *__restrict__ part, int nb, double *__restrict__ out6) {
    __shared__ double sm[6][256];
    double mn[3] = {1e300, 1e300, 1e300}, mx[3] = {-1e300, -1e300, -1e300};
    for (int b = threadIdx.x; b < nb; b += 256)
        for (int a = 0; a < 3; a++) { mn[a] = fmin(mn[a], part[b * 6 + a]); mx[a] = fmax(mx[a], part[b * 6 + 3 + a]); }
    for (int a = 0; a < 3; a++) { sm[a][threadIdx.x] = mn[a]; sm[3 + a][threadIdx.x] = mx[a]; }
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s)
            for (int a = 0; a < 3; a++) {
                sm[a][threadIdx.x] = fmin(sm[a][threadIdx.x], sm[a][threadIdx.x + s]);
                sm[3 + a][threadIdx.x] = fmax(sm[3 + a][threadIdx.x], sm[3 + a][threadIdx.x + s]);
            }
        __syncthreads();
    }
    if (threadIdx.x < 6) out6[threadIdx.x] = sm[threadIdx.x][0];
}

// ------------------------------------------------------------------------------------------------ keys
// KEY = unsigned (the key space fits 32 bits: half the bytes through every radix pass) or unsigned long long
template <class KEY>
__global__ void __launch_bounds__(256) k_cell_keys(const double *__restrict__ p, int64_t n, double ox, double oy, double oz,
                                                   double cell, int nx, int ny, int nz, int key_order,
                                                   KEY *__restrict__ keys, int *__restrict__ vals) {
    int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int cx, cy, cz;
    if (key_order == 1) {  // voxel keys: the legacy index is floor((p - origin) / voxel) with a true division
        cx = (int)floor((p[i * 3] - ox) / cell); cy = (int)floor((p[i * 3 + 1] - oy) / cell); cz = (int)floor((p[i * 3 + 2] - oz) / cell);
    } else if (key_order == 3) {  // tensor voxel keys: floor(float(p) / float(voxel)) in float32, grid origin 0; ox..oz = smallest key
        const float v = (float)cell;
        cx = (int)((long long)floorf((float)p[i * 3] / v) - (long long)ox);
        cy = (int)((long long)floorf((float)p[i * 3 + 1] / v) - (long long)oy);
        cz = (int)((long long)floorf((float)p[i * 3 + 2] / v) - (long long)oz);
    } else {               // search grid: must agree with cell_coord() used by the queries
        const double inv = 1.0 / cell;
        cx = cell_coord(p[i * 3], ox, inv); cy = cell_coord(p[i * 3 + 1], oy, inv); cz = cell_coord(p[i * 3 + 2], oz, inv);
    }
    cx = min(max(cx, 0), nx - 1); cy = min(max(cy, 0), ny - 1); cz = min(max(cz, 0), nz - 1);
    // key_order 0: x fastest (search grid); 1: z fastest (voxel output in lexicographic (kx,ky,kz) order);
    // 2: Morton code of the cell coordinates (query ordering: consecutive points stay compact in all three axes)
    unsigned long long k;
    if (key_order == 2) {
        auto spread = [](unsigned long long v) {  // 21 bits -> every third bit
            v &= 0x1fffffull;
            v = (v | v << 32) & 0x1f00000000ffffull;
            v = (v | v << 16) & 0x1f0000ff0000ffull;
            v = (v | v << 8) & 0x100f00f00f00f00full;
            v = (v | v << 4) & 0x10c30c30c30c30c3ull;
            v = (v | v << 2) & 0x1249249249249249ull;
            return v;
        };
        k = spread((unsigned long long)cx) | spread((unsigned long long)cy) << 1 | spread((unsigned long long)cz) << 2;
    } else {
        k = key_order == 0 ? ((unsigned long long)cz * ny + cy) * nx + cx : ((unsigned long long)cx * ny + cy) * nz + cz;   // 1 and 3: z fastest
    }
    keys[i] = (KEY)k;
    vals[i] = (int)i;
}

// population of every cell: the last point of a run of equal (sorted) keys knows the run length
template <class KEY>
__global__ void __launch_bounds__(256) k_cell_counts(const KEY *__restrict__ keys, int64_t n, int *__restrict__ run_start,
                                                     int *__restrict__ counts) {
    int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const KEY k = keys[i];
    if (i == 0 || keys[i - 1] != k) run_start[k] = (int)i;
}
template <class KEY>
__global__ void __launch_bounds__(256) k_cell_counts2(const KEY *__restrict__ keys, int64_t n, const int *__restrict__ run_start,
                                                      int *__restrict__ counts) {
    int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const KEY k = keys[i];
    if (i == n - 1 || keys[i + 1] != k) counts[k] = (int)i + 1 - run_start[k];
}

__global__ void __launch_bounds__(256) k_gather3(const double *__restrict__ src, const int *__restrict__ idx, int64_t n, double *__restrict__ dst) {
    int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int j = idx[i];
    dst[i * 3] = src[(int64_t)j * 3]; dst[i * 3 + 1] = src[(int64_t)j * 3 + 1]; dst[i * 3 + 2] = src[(int64_t)j * 3 + 2];
}

// ================================================================================== hand-written exclusive scan (int32 / packed 64)
// Reduce-then-scan in two launches: k_scan_sums leaves one sum per 4096-element tile; k_scan_apply first adds up the tile sums in
// front of its own tile (the list is short: 2 000 tiles for an 8 MP image, read from L2) and then scans its tile.  Integer adds:
// the result does not depend on the order, so it is deterministic.  T = int (flags, cell populations) or unsigned long long
// (two counters packed: points in the low word, runs in the high word; both stay below 2^31 so no carry crosses).
constexpr int SCAN_T = 256, SCAN_I = 16, SCAN_TILE = SCAN_T * SCAN_I;
// MAXOP: the running maximum instead of the running sum (values >= 0; used to carry "points so far" across empty table lines)
template <class T, bool MAXOP = false>
__device__ __forceinline__ T scan_op(T a, T b) { return MAXOP ? (a > b ? a : b) : a + b; }
template <class T, bool MAXOP = false>
__device__ __forceinline__ T wave_incl_scan(T v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T t = __shfl_up(v, o);
        if (lane >= o) v = scan_op<T, MAXOP>(v, t);
    }
    return v;
}
// one value per thread of a 256-thread workgroup -> exclusive prefix; *total = workgroup sum
template <class T, bool MAXOP = false>
__device__ __forceinline__ T block_excl_scan(T v, T *total, T *ws /* 4 entries of LDS */) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const T incl = wave_incl_scan<T, MAXOP>(v, lane);
    if (lane == 63) ws[w] = incl;
    __syncthreads();
    T off = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) { if (i < w) off = scan_op<T, MAXOP>(off, ws[i]); tot = scan_op<T, MAXOP>(tot, ws[i]); }
    __syncthreads();
    *total = tot;
    if (MAXOP) {   // exclusive = the inclusive value of the lane before (0 for the first lane of the wave), joined with the waves before
        T prev = __shfl_up(incl, 1);
        if (lane == 0) prev = 0;
        return scan_op<T, true>(off, prev);
    }
    return off + incl - v;
}
// 16 consecutive elements of a thread as 16-byte accesses when the whole group is inside the array (the arrays come from the arena:
// 256-byte aligned, and base is a multiple of 16 elements)
template <class T>
__device__ __forceinline__ void scan_load16(const T *__restrict__ in, int64_t base, int64_t n, T v[SCAN_I]) {
    if (base + SCAN_I <= n) {
        constexpr int PER = 16 / sizeof(T);
        typedef T vec_t __attribute__((ext_vector_type(PER)));
        const vec_t *p = reinterpret_cast<const vec_t *>(in + base);
#pragma unroll
        for (int q = 0; q < SCAN_I / PER; q++) {
            const vec_t t = p[q];
#pragma unroll
            for (int c = 0; c < PER; c++) v[q * PER + c] = t[c];
        }
    } else {
#pragma unroll
        for (int j = 0; j < SCAN_I; j++) v[j] = base + j < n ? in[base + j] : (T)0;
    }
}
template <class T, bool MAXOP = false>
__global__ void __launch_bounds__(SCAN_T) k_scan_sums(const T *__restrict__ in, int64_t n, T *__restrict__ part) {
    __shared__ T ws[4];
    const int64_t base = (int64_t)blockIdx.x * SCAN_TILE + (int64_t)threadIdx.x * SCAN_I;
    T v[SCAN_I], s = 0;
    scan_load16<T>(in, base, n, v);
#pragma unroll
    for (int j = 0; j < SCAN_I; j++) s = scan_op<T, MAXOP>(s, v[j]);
    T tot;
    (void)block_excl_scan<T, MAXOP>(s, &tot, ws);
    if (threadIdx.x == 0) part[blockIdx.x] = tot;
}
// hi_max (T = unsigned long long only): the largest HIGH word of any input element (runs per bucket), by atomicMax
template <class T, bool MAXOP = false>
__global__ void __launch_bounds__(SCAN_T) k_scan_apply(const T *__restrict__ in, int64_t n, const T *__restrict__ part, T *__restrict__ out,
                                                       int *__restrict__ lo_out, int *__restrict__ hi_max) {
    __shared__ T ws[4];
    T acc = 0;
    for (int b = threadIdx.x; b < (int)blockIdx.x; b += SCAN_T) acc = scan_op<T, MAXOP>(acc, part[b]);
    T tile_off;
    (void)block_excl_scan<T, MAXOP>(acc, &tile_off, ws);
    const int64_t base = (int64_t)blockIdx.x * SCAN_TILE + (int64_t)threadIdx.x * SCAN_I;
    T v[SCAN_I], s = 0;
    int hm = 0;
    scan_load16<T>(in, base, n, v);
#pragma unroll
    for (int j = 0; j < SCAN_I; j++) {
        if (sizeof(T) == 8) hm = max(hm, (int)((unsigned long long)v[j] >> 32));
        s = scan_op<T, MAXOP>(s, v[j]);
    }
    T tot;
    T run = scan_op<T, MAXOP>(tile_off, block_excl_scan<T, MAXOP>(s, &tot, ws));
    if (base + SCAN_I <= n && !lo_out) {
        constexpr int PER = 16 / sizeof(T);
        typedef T vec_t __attribute__((ext_vector_type(PER)));
        vec_t *p = reinterpret_cast<vec_t *>(out + base);
#pragma unroll
        for (int q = 0; q < SCAN_I / PER; q++) {
            vec_t t;
#pragma unroll
            for (int c = 0; c < PER; c++) { t[c] = run; run = scan_op<T, MAXOP>(run, v[q * PER + c]); }
            p[q] = t;
        }
    } else {
#pragma unroll
        for (int j = 0; j < SCAN_I; j++) {
            if (base + j < n) {
                out[base + j] = run;
                if (lo_out) lo_out[base + j] = (int)(unsigned)run;
            }
            run = scan_op<T, MAXOP>(run, v[j]);
        }
    }
    if (sizeof(T) == 8 && hi_max) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) hm = max(hm, __shfl_xor(hm, o));
        if ((threadIdx.x & 63) == 0 && hm > 0) atomicMax(hi_max, hm);
    }
}

// ================================================================================== stable counting sort by cell key, run based
// Sorts point indices by (key, index) WITHOUT a radix pass.  Consecutive points with the same key (the pixels of an image row that
// fall into one voxel; the members of a voxelised cloud in key order) form a RUN; a run is one record (key, first index,
// length).  k_cs_runs detects runs inside every wave (64 consecutive points), counts per BUCKET -- a coarse prefix of the key: the
// (kx, ky) column of a z-fastest voxel key, the high bits of a Morton or x-fastest key -- how many runs and points it receives
// (one 64-bit atomic per run head: runs << 32 | points) and hands every run a slot in a global list.  After a scan of the bucket
// table, k_cs_place files every run under its bucket, k_cs_rank gives every run its final position by counting, among the runs
// of ITS bucket, the points of those that sort before it by (key, first index) -- the only quadratic step, in runs per bucket
// (tens) -- and k_cs_emit writes every point to final base + offset inside its run.  Arrival order (the atomics) only picks
// scratch slots: the result is the unique stable order, identical to a stable radix sort.  The bucket table is small (L2
// resident); the point arrays are read and written once each.
template <class KEY>
struct CsRun { KEY key; int start, len; unsigned bucket; int gid; };
struct CsGeom { double ox, oy, oz, cell; int nx, ny, nz, key_order, shift; unsigned long long div; };   // bucket = key >> shift, or key / div when shift < 0

template <class KEY>
__device__ __forceinline__ void cs_key(const double *__restrict__ p, int64_t i, const CsGeom &g, KEY &full, unsigned &bucket) {
    int cx, cy, cz;
    if (g.key_order == 1) {  // voxel keys: the legacy index is floor((p - origin) / voxel) with a true division
        cx = (int)floor((p[i * 3] - g.ox) / g.cell); cy = (int)floor((p[i * 3 + 1] - g.oy) / g.cell); cz = (int)floor((p[i * 3 + 2] - g.oz) / g.cell);
    } else if (g.key_order == 3) {  // tensor voxel keys: floor(float(p) / float(voxel)) in float32, grid origin 0; ox..oz = smallest key
        const float v = (float)g.cell;
        cx = (int)((long long)floorf((float)p[i * 3] / v) - (long long)g.ox);
        cy = (int)((long long)floorf((float)p[i * 3 + 1] / v) - (long long)g.oy);
        cz = (int)((long long)floorf((float)p[i * 3 + 2] / v) - (long long)g.oz);
    } else {               // search grid: must agree with cell_coord() used by the queries
        const double inv = 1.0 / g.cell;
        cx = cell_coord(p[i * 3], g.ox, inv); cy = cell_coord(p[i * 3 + 1], g.oy, inv); cz = cell_coord(p[i * 3 + 2], g.oz, inv);
    }
    cx = min(max(cx, 0), g.nx - 1); cy = min(max(cy, 0), g.ny - 1); cz = min(max(cz, 0), g.nz - 1);
    unsigned long long k;
    if (g.key_order == 2) {
        auto spread = [](unsigned long long v) {  // 21 bits -> every third bit
            v &= 0x1fffffull;
            v = (v | v << 32) & 0x1f00000000ffffull;
            v = (v | v << 16) & 0x1f0000ff0000ffull;
            v = (v | v << 8) & 0x100f00f00f00f00full;
            v = (v | v << 4) & 0x10c30c30c30c30c3ull;
            v = (v | v << 2) & 0x1249249249249249ull;
            return v;
        };
        k = spread((unsigned long long)cx) | spread((unsigned long long)cy) << 1 | spread((unsigned long long)cz) << 2;
        bucket = (unsigned)(k >> g.shift);
    } else if (g.key_order == 0) {
        k = ((unsigned long long)cz * g.ny + cy) * g.nx + cx;
        bucket = (unsigned)(k >> g.shift);
    } else {   // 1 and 3: z fastest; bucket = a stretch of g.div consecutive keys (a piece of a (kx, ky) column)
        k = ((unsigned long long)cx * g.ny + cy) * g.nz + cz;
        bucket = sizeof(KEY) == 4 ? (unsigned)k / (unsigned)g.div : (unsigned)(k / g.div);
    }
    full = (KEY)k;
}

template <class KEY>
__global__ void __launch_bounds__(256) k_cs_runs(const double *__restrict__ p, int64_t n, CsGeom g, KEY *__restrict__ keys, int *__restrict__ gid_of,
                                                 unsigned long long *__restrict__ cnt, CsRun<KEY> *__restrict__ runs) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool valid = i < n;
    KEY key = 0;
    unsigned bucket = 0;
    if (valid) cs_key<KEY>(p, i, g, key, bucket);
    const KEY prev = __shfl_up(key, 1);
    const bool head = valid && (lane == 0 || prev != key);
    const unsigned long long hm = __ballot(head), vm = __ballot(valid);
    if (vm == 0) return;
    const unsigned long long upto = (2ull << lane) - 1ull;           // bits 0 .. lane (lane 63: all ones)
    const int hp = 63 - __clzll((long long)(hm & upto));              // lane of my run's head (lane 0 is always a head)
    const unsigned long long above = hm & ~upto;
    const int nxt = above ? __ffsll((long long)above) - 1 : __popcll(vm);   // valid lanes are a prefix of the wave
    // a run is named by the index of its first point (no global counter: one address hit by every wave of the grid serialises)
    if (head) {
        const int len = nxt - lane;
        const unsigned long long old = atomicAdd(&cnt[bucket], (1ull << 32) | (unsigned long long)len);
        CsRun<KEY> r;
        r.key = key; r.start = (int)i; r.len = len; r.bucket = bucket;
        r.gid = (int)(old >> 32);      // arrival number of the run inside its bucket (picks a scratch slot only) until k_cs_place
        runs[i] = r;
    }
    if (valid) { keys[i] = key; gid_of[i] = (int)i - (lane - hp); }
}
// files every run under its bucket: placed[run_start(bucket) + arrival number]; one thread per point, run heads act
template <class KEY>
__global__ void __launch_bounds__(256) k_cs_place(const CsRun<KEY> *__restrict__ runs, const int *__restrict__ gid_of, int64_t n,
                                                  const unsigned long long *__restrict__ start, CsRun<KEY> *__restrict__ placed) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n || gid_of[i] != (int)i) return;
    CsRun<KEY> r = runs[i];
    const int slot = (int)(start[r.bucket] >> 32) + r.gid;
    r.gid = (int)i;
    placed[slot] = r;
}
// final position of every run: points of its bucket's runs that sort before it by (key, first index).  Wave-cooperative: the 64
// runs of a wave lie in consecutive buckets, so the union of their buckets' run lists is ONE contiguous stretch of `placed`; the
// wave reads it 64 records at a time (one coalesced load) and every lane tests all 64 through v_readlane (uniform index), counting
// only the records of its own bucket.  Cost per wave: union length x ~8 instructions, whatever the split into buckets.
__device__ __forceinline__ unsigned long long readlane_u64(unsigned long long v, int l) {
    const unsigned lo = __builtin_amdgcn_readlane((int)(unsigned)v, l), hi = __builtin_amdgcn_readlane((int)(unsigned)(v >> 32), l);
    return (unsigned long long)hi << 32 | lo;
}
template <class KEY>
__global__ void __launch_bounds__(256) k_cs_rank(const CsRun<KEY> *__restrict__ placed, int nruns, const unsigned long long *__restrict__ start,
                                                 int *__restrict__ final_base, const unsigned long long *__restrict__ d_total,
                                                 const int *__restrict__ d_maxruns, int max_runs_allowed) {
    // deferred mode (d_total != NULL): the host has NOT read the run count and the fallback test yet -- they travel with the
    // caller's next read-back -- so the grid covers the upper bound (one run per point), the count comes from device memory, and
    // a bucket population the quadratic step below must not be asked to rank makes the whole kernel a no-op (the host then
    // discards this sort and runs the radix sort)
    if (d_total) {
        if (*d_maxruns > max_runs_allowed) return;
        nruns = (int)(*d_total >> 32);
    }
    const int s = blockIdx.x * 256 + threadIdx.x;   // nruns = high word of the scan total, read by the host together with the fallback test
    if ((s & ~63) >= nruns) return;                  // whole wave beyond the list
    const bool valid = s < nruns;
    const CsRun<KEY> me = placed[valid ? s : nruns - 1];
    const unsigned long long b0 = start[me.bucket], b1 = start[me.bucket + 1];
    const int rb = (int)(b0 >> 32), re = (int)(b1 >> 32);
    int acc = (int)(unsigned)b0;
    const int u0 = __builtin_amdgcn_readfirstlane(rb);
    int u1 = re;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) u1 = max(u1, __shfl_xor(u1, o));
    u1 = __builtin_amdgcn_readfirstlane(u1);
    const int lane = threadIdx.x & 63;
    for (int c = u0; c < u1; c += 64) {
        const CsRun<KEY> o = placed[min(c + lane, nruns - 1)];
        const int lim = min(64, u1 - c);
        for (int t = 0; t < lim; t++) {
            KEY ok;
            if (sizeof(KEY) == 8) ok = (KEY)readlane_u64((unsigned long long)o.key, t);
            else ok = (KEY)(unsigned)__builtin_amdgcn_readlane((int)(unsigned)o.key, t);
            const int os = __builtin_amdgcn_readlane(o.start, t), ol = __builtin_amdgcn_readlane(o.len, t);
            const int j = c + t;
            const bool less = ok < me.key || (ok == me.key && os < me.start);
            acc += (j >= rb && j < re && less) ? ol : 0;
        }
    }
    if (valid) final_base[me.gid] = acc;
}
// every point to its final slot; optionally the gathered coordinates as well (the cell-sorted copy a search grid needs)
template <class KEY>
__global__ void __launch_bounds__(256) k_cs_emit(const KEY *__restrict__ keys, const int *__restrict__ gid_of, const int *__restrict__ final_base, int64_t n, KEY *__restrict__ keys_out, int *__restrict__ idx_out,
                                                 const double *__restrict__ pts, double *__restrict__ sorted, const int *__restrict__ d_maxruns, int max_runs_allowed) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if (d_maxruns && *d_maxruns > max_runs_allowed) return;           // deferred mode: k_cs_rank did not run, final_base holds nothing
    const int g = gid_of[i];                                         // = index of the first point of my run
    const int64_t o = (int64_t)final_base[g] + ((int)i - g);
    keys_out[o] = keys[i];
    idx_out[o] = (int)i;
    if (sorted) { sorted[o * 3] = pts[i * 3]; sorted[o * 3 + 1] = pts[i * 3 + 1]; sorted[o * 3 + 2] = pts[i * 3 + 2]; }
}

// ================================================================================== two-level cell table (GridView::l1 / l2)
// Built from the SORTED keys.  k_line_mark: which lines hold a point in their 36-cell reach, and, per line, one past the sorted
// slot of its last point (so that an exclusive running maximum over the lines gives "points before this line").  k_line_l1: the
// first level.  k_line_fill: every run start i (first slot of a cell c, previous occupied cell p) owns the cells (p, c]: their
// cstart is i; it writes that value into the materialised lines that reach into (p, c] -- those are the lines that contain p or
// c in their 36-cell reach (a materialised line holds an occupied cell q; for an entry cc <= q the owner's c lies in [cc, q], for
// cc > q its p lies in [q, cc): inside the line either way), at most four lines per run start.  Slot n is the virtual last
// run start (c = +infinity).
template <class KEY>
__global__ void __launch_bounds__(256) k_line_mark(const KEY *__restrict__ keys, int64_t n, int *__restrict__ mark, int *__restrict__ last1) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const long long c = (long long)keys[i];
    if (i == 0 || (long long)keys[i - 1] != c) {
        mark[c >> CL_SHIFT] = 1;
        if ((c & 31) < CL_STRIDE - 32 && c >= 32) mark[(c >> CL_SHIFT) - 1] = 1;
    }
    if (i == n - 1 || ((long long)keys[i + 1] >> CL_SHIFT) != (c >> CL_SHIFT)) last1[c >> CL_SHIFT] = (int)i + 1;
}
__global__ void __launch_bounds__(256) k_line_l1(const int *__restrict__ mark, const int *__restrict__ ids, const int *__restrict__ before,
                                                 int64_t nl, int *__restrict__ l1) {
    const int64_t L = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (L >= nl) return;
    l1[L] = mark[L] ? -(ids[L] + 1) : before[L];
}
template <class KEY>
__global__ void __launch_bounds__(256) k_line_fill(const KEY *__restrict__ keys, int64_t n, const int *__restrict__ l1, int64_t nl, int *__restrict__ l2) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i > n) return;
    const long long p = i > 0 ? (long long)keys[i - 1] : -1, c = i < n ? (long long)keys[i] : (long long)nl * 32 + CL_STRIDE;
    if (i < n && i > 0 && p == c) return;            // not a run start
    long long cand[4] = {(p >> CL_SHIFT) - 1, p >> CL_SHIFT, (c >> CL_SHIFT) - 1, c >> CL_SHIFT};   // (p = -1: lines -2 and -1, skipped)
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const long long L = cand[q];
        bool dup = false;
#pragma unroll
        for (int r = 0; r < 4; r++) dup = dup || (r < q && cand[r] == L);
        if (dup || L < 0 || L >= nl) continue;
        const int v = l1[L];
        if (v >= 0) continue;                        // not materialised
        int *e = l2 + (int64_t)(-v - 1) * CL_STRIDE;
        const long long c0 = L * 32;
        const int w0 = (int)max(p + 1 - c0, 0ll), w1 = (int)min(c - c0, (long long)CL_STRIDE - 1);
        for (int w = w0; w <= w1; w++) e[w] = (int)i;
    }
}

// ------------------------------------------------------------------------------------------------ voxel
// segment heads of the sorted key array -> compact list of segment starts (one output voxel per segment)
template <class KEY>
__global__ void __launch_bounds__(256) k_seg_flags(const KEY *__restrict__ keys, int64_t n, int *__restrict__ flags) {
    int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    flags[i] = (i == 0 || keys[i - 1] != keys[i]) ? 1 : 0;
}
__global__ void __launch_bounds__(256) k_seg_starts(const int *__restrict__ flags, const int *__restrict__ scan, int64_t n, int *__restrict__ starts) {
    int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if (flags[i]) starts[scan[i]] = (int)i;
}
// Voxel means: sequential sums in ORIGINAL point order (the sort is stable), exactly like the accumulate-then-divide of the legacy
// VoxelDownSample (T = double) / of the tensor method (T = float: members rounded to float32, float32 sums, float32 count).
// One thread per voxel keeps the order, and the kernel then lasts as long as its most populated voxel's chain of round trips
// (1 400 members in the near field of an 8 MP view: 175 rounds of 8, 0.30 ms for a kernel that moves 0.2 GB).  So voxels with more
// than VM_BIG members are only LISTED by k_voxel_mean_t (one wave-aggregated atomic per wave) and summed by k_voxel_mean_big, a wave
// per voxel: 64 members per round trip (coalesced index read, 64 gathers in flight), added in order through v_readlane -- every
// lane carries the same running sum, the additions are the voxel's own sequential chain, nothing else waits on them.
// (A form that staged 64 voxels' members through LDS windows was measured 3x SLOWER: where voxels are larger than the window only
// one lane walks at a time; 16 members per thread and round trip instead of 8: 2x slower.)
constexpr int VM_BIG = 192;
// What member j of the index list contributes is the kernels' LD parameter: fetch(j) issues the member's loads and returns what
// they bring, value() turns that into the three summands -- two steps, so that a kernel can keep several members' loads in
// flight before the first conversion waits for one.  MemberXyz: row j of a float64 [n,3] array.
struct MemberXyz {
    struct Raw { double x, y, z; };
    const double *__restrict__ a;
    __device__ __forceinline__ Raw fetch(int64_t j) const { return Raw{a[j * 3], a[j * 3 + 1], a[j * 3 + 2]}; }
    template <class T>
    static __device__ __forceinline__ void value(const Raw &m, T &x, T &y, T &z) { x = (T)m.x; y = (T)m.y; z = (T)m.z; }
};
// MemberColor<CN>: the colour of the pixel that compacted point j came from (pix[j], the row-major index k_reproject wrote), read
// from a uint8 image with CN = 1 or 3 interleaved channels: (double)byte / 255.0 as k_backproject, in r, g, b order (bgr: the
// pixel's bytes are b, g, r).  No [w*h,3] float64 colour array ever exists: the means are summed from the bytes.  CN is a template
// parameter so that a pixel's bytes sit at constant offsets from one address.  (Read off the gfx950 listing, hipcc -S, of
// k_voxel_mean_t: with run-time channel offsets a thread's eight members were fetched channel by channel, three dependent groups
// of eight byte loads; in this form a 3-channel pixel is one 16-bit and one 8-bit load and the eight members go out as two groups
// of eight loads.  The two forms were not timed against each other.)
struct ColorImage { const unsigned char *img; int w, stride, bgr; };
template <int CN>
struct MemberColor {
    struct Raw { unsigned char v[CN]; };
    const int *__restrict__ pix;
    ColorImage c;
    __device__ __forceinline__ Raw fetch(int64_t j) const {
        const int p = pix[j];
        const unsigned char *__restrict__ q = c.img + (int64_t)(p / c.w) * c.stride + (p % c.w) * CN;
        Raw m;
#pragma unroll
        for (int k = 0; k < CN; k++) m.v[k] = q[k];
        return m;
    }
    template <class T>
    __device__ __forceinline__ void value(const Raw &m, T &r, T &g, T &b) const {
        const unsigned char v0 = m.v[0], v1 = m.v[CN / 2], v2 = m.v[CN - 1];
        r = (T)((double)(c.bgr ? v2 : v0) / 255.0); g = (T)((double)v1 / 255.0); b = (T)((double)(c.bgr ? v0 : v2) / 255.0);
    }
};
template <class T, class LD>
__global__ void __launch_bounds__(256) k_voxel_mean_t(LD ld, const int *__restrict__ idx, const int *__restrict__ starts,
                                                      int64_t nseg, int64_t n, double *__restrict__ out, int *__restrict__ big_list,
                                                      int *__restrict__ big_count) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool live = s < nseg;
    const int b = live ? starts[s] : 0, e = live ? (s + 1 < nseg ? starts[s + 1] : (int)n) : 0;
    const bool big = e - b > VM_BIG;
    const unsigned long long bm = __ballot(big);
    if (bm) {   // wave-uniform
        const int lane = threadIdx.x & 63;
        int base = 0;
        if (lane == 0) base = atomicAdd(big_count, __popcll(bm));
        base = __shfl(base, 0);
        if (big) big_list[base + __popcll(bm & ((1ull << lane) - 1ull))] = (int)s;
    }
    if (!live || big) return;
    T x = 0, y = 0, z = 0;
    for (int i0 = b; i0 < e; i0 += 8) {
        int64_t j[8];
        typename LD::Raw m[8];
        T X[8], Y[8], Z[8];
#pragma unroll
        for (int u = 0; u < 8; u++) j[u] = idx[min(i0 + u, e - 1)];
#pragma unroll
        for (int u = 0; u < 8; u++) m[u] = ld.fetch(j[u]);
#pragma unroll
        for (int u = 0; u < 8; u++) ld.value(m[u], X[u], Y[u], Z[u]);
#pragma unroll
        for (int u = 0; u < 8; u++)
            if (i0 + u < e) { x += X[u]; y += Y[u]; z += Z[u]; }
    }
    const T c = (T)(e - b);
    out[s * 3] = (double)(x / c); out[s * 3 + 1] = (double)(y / c); out[s * 3 + 2] = (double)(z / c);
}
// the same sums over the points IN SORTED ORDER (the sort wrote them, k_cs_emit): a voxel's members are one contiguous stretch, so
// a lane streams whole cache lines instead of gathering 24 bytes from each; the next eight members are requested before the
// current eight are added
template <class T, int R>
__global__ void __launch_bounds__(256) k_voxel_mean_sorted(const double *__restrict__ sp, const int *__restrict__ starts, int64_t nseg, int64_t n,
                                                           double *__restrict__ out) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= nseg) return;
    const int b = starts[s], e = s + 1 < nseg ? starts[s + 1] : (int)n, m = e - b;
    const double *__restrict__ p = sp + (int64_t)b * 3;
    T x = 0, y = 0, z = 0;
    double cur[3 * R], nxt[3 * R];
#pragma unroll
    for (int u = 0; u < R; u++) {
        const int64_t q = (int64_t)min(u, m - 1) * 3;
        cur[u * 3] = p[q]; cur[u * 3 + 1] = p[q + 1]; cur[u * 3 + 2] = p[q + 2];
    }
    for (int i0 = 0; i0 < m; i0 += R) {
#pragma unroll
        for (int u = 0; u < R; u++) {
            const int64_t q = (int64_t)min(i0 + R + u, m - 1) * 3;
            nxt[u * 3] = p[q]; nxt[u * 3 + 1] = p[q + 1]; nxt[u * 3 + 2] = p[q + 2];
        }
#pragma unroll
        for (int u = 0; u < R; u++)
            if (i0 + u < m) { x += (T)cur[u * 3]; y += (T)cur[u * 3 + 1]; z += (T)cur[u * 3 + 2]; }
#pragma unroll
        for (int u = 0; u < 3 * R; u++) cur[u] = nxt[u];
    }
    const T c = (T)m;
    out[s * 3] = (double)(x / c); out[s * 3 + 1] = (double)(y / c); out[s * 3 + 2] = (double)(z / c);
}
__device__ __forceinline__ double readlane_t(double v, int l) { return __longlong_as_double((long long)readlane_u64((unsigned long long)__double_as_longlong(v), l)); }
__device__ __forceinline__ float readlane_t(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }
template <class T, class LD>
__global__ void __launch_bounds__(64) k_voxel_mean_big(LD ld, const int *__restrict__ idx, const int *__restrict__ starts,
                                                       int64_t nseg, int64_t n, double *__restrict__ out, const int *__restrict__ big_list,
                                                       const int *__restrict__ big_count) {
    const int lane = threadIdx.x, nbig = *big_count;
    for (int q = blockIdx.x; q < nbig; q += gridDim.x) {
        const int64_t s = big_list[q];
        const int b = starts[s], e = s + 1 < nseg ? starts[s + 1] : (int)n;
        T x = 0, y = 0, z = 0;
        T X, Y, Z;
        ld.value(ld.fetch(idx[min(b + lane, e - 1)]), X, Y, Z);
        for (int c = b; c < e; c += 64) {
            const typename LD::Raw mn = ld.fetch(idx[min(c + 64 + lane, e - 1)]);   // next chunk in flight while this one is added
            const int lim = min(64, e - c);
            for (int t = 0; t < lim; t++) { x += readlane_t(X, t); y += readlane_t(Y, t); z += readlane_t(Z, t); }
            ld.value(mn, X, Y, Z);
        }
        if (lane == 0) {
            const T cnt = (T)(e - b);
            out[s * 3] = (double)(x / cnt); out[s * 3 + 1] = (double)(y / cnt); out[s * 3 + 2] = (double)(z / cnt);
        }
    }
}
// ------------------------------------------------------------------------------------------------ search
// visits the cells of Chebyshev shell s around (cx,cy,cz); F(slot_begin, slot_end) is called per non-empty cell
template <class F>
__device__ __forceinline__ void for_shell(const GridView &g, int cx, int cy, int cz, int s, F &&f) {
    for (int dz = -s; dz <= s; dz++) {
        int z = cz + dz;
        if (z < 0 || z >= g.nz) continue;
        for (int dy = -s; dy <= s; dy++) {
            int y = cy + dy;
            if (y < 0 || y >= g.ny) continue;
            const bool face = (dz == -s || dz == s || dy == -s || dy == s);
            const int step = face ? 1 : 2 * s;  // interior rows of the shell only touch dx = -s and dx = +s
            for (int dx = -s; dx <= s; dx += (step > 0 ? step : 1)) {
                int x = cx + dx;
                if (x < 0 || x >= g.nx) continue;
                int64_t c = ((int64_t)z * g.ny + y) * g.nx + x;
                int b = cs1(g, c), e = cs1(g, c + 1);
                if (e > b) f(b, e);
            }
        }
    }
}

// the 3x3x3 block around (cx,cy,cz) as NINE runs: the three cells of an x-row are contiguous in the sorted point array
template <class F>
__device__ __forceinline__ void for_block3(const GridView &g, int cx, int cy, int cz, F &&f) {
    const int x0 = max(cx - 1, 0), x1 = min(cx + 1, g.nx - 1);
    if (x0 > x1) return;
    for (int dz = -1; dz <= 1; dz++) {
        const int z = cz + dz;
        if (z < 0 || z >= g.nz) continue;
        for (int dy = -1; dy <= 1; dy++) {
            const int y = cy + dy;
            if (y < 0 || y >= g.ny) continue;
            const int64_t row = ((int64_t)z * g.ny + y) * g.nx;
            const int b = cs1(g, row + x0), e = cs1(g, row + x1 + 1);
            if (e > b) f(b, e);
        }
    }
}

// Shell s >= 2 walked by x-rows with pruning.  A row on a face of the shell is ONE contiguous run of the sorted point array
// (two table entries instead of 2 (2s+1)), trimmed in x to the cells that can still hold a useful point; a row inside the
// shell only contributes its two end cells; rows and cells whose nearest face is further than bound() are skipped.
// bound() is the squared distance beyond which a candidate is useless to the caller (re-read for every row, so it tightens
// as the caller's result improves); the comparison is strict and shrunk by more than the rounding of the cell faces, so a
// point at exactly the bound is still visited (ties are decided by the caller's total order).
template <class Bound, class F>
__device__ __forceinline__ void for_shell_rows(const GridView &g, double px, double py, double pz, int cx, int cy, int cz, int s,
                                               Bound &&bound, F &&visit) {
    constexpr double SLK = 1.0 - 1e-9;
    auto slab = [&](double q, double o, int c) {   // distance from coordinate q to the slab of cell c along one axis (0 inside)
        const double lo = o + (double)c * g.cell, hi = lo + g.cell;
        return q < lo ? lo - q : (q > hi ? q - hi : 0.0);
    };
    // rows are taken centre-out (0, -1, +1, -2, ...): near rows tighten the bound before the far ones are looked at
    for (int iz = 0; iz <= 2 * s; iz++) {
        const int dz = (iz & 1) ? -((iz + 1) >> 1) : (iz >> 1);
        const int z = cz + dz;
        if (z < 0 || z >= g.nz) continue;
        const double sz = slab(pz, g.oz, z);
        if (sz * sz * SLK > bound()) continue;
        for (int iy = 0; iy <= 2 * s; iy++) {
            const int dy = (iy & 1) ? -((iy + 1) >> 1) : (iy >> 1);
            const int y = cy + dy;
            if (y < 0 || y >= g.ny) continue;
            const double sy = slab(py, g.oy, y), syz = sy * sy + sz * sz, bnd = bound();
            if (syz * SLK > bnd) continue;
            const int64_t row = ((int64_t)z * g.ny + y) * g.nx;
            if (dz == -s || dz == s || dy == -s || dy == s) {
                // cells further than kx from the query's cell lie at least (kx - 1) * cell away in x
                const double rx = sqrt(fmax(bnd - syz * SLK, 0.0)) * g.inv_cell;
                const int kx = rx < (double)s ? (int)rx + 1 : s;
                const int x0 = max(cx - min(kx, s), 0), x1 = min(cx + min(kx, s), g.nx - 1);
                if (x0 > x1) continue;
                const int b = cs1(g, row + x0), e = cs1(g, row + x1 + 1);
                if (e > b) visit(b, e);
            } else {
#pragma unroll
                for (int side = 0; side < 2; side++) {
                    const int x = side ? cx + s : cx - s;
                    if (x < 0 || x >= g.nx) continue;
                    const double sx = slab(px, g.ox, x);
                    if ((sx * sx + syz) * SLK > bound()) continue;
                    const int b = cs1(g, row + x), e = cs1(g, row + x + 1);
                    if (e > b) visit(b, e);
                }
            }
        }
    }
}

// max shells needed to cover the whole grid from a clamped centre
__device__ __forceinline__ int max_shell(const GridView &g, int cx, int cy, int cz) {
    int m = max(max(cx, g.nx - 1 - cx), max(max(cy, g.ny - 1 - cy), max(cz, g.nz - 1 - cz)));
    return max(m, 0);
}

// ---- k nearest (<= k, distance < radius if radius > 0), sorted ascending, in LDS columns [slot][thread]
// Selection keeps the list as a binary MAX-HEAP in the total order (d2, original index) while candidates stream by: the root
// is the current k-th neighbour, an accepted candidate replaces it and sifts down (<= log2 k levels).  A sorted insertion
// costs every lane of the wave the longest shift chain of any lane at every candidate (PMC of that form: 71 k instructions
// per 64 queries, 53 % of them scalar loop control; k_normals 2.9 ms at 1 M points, 1.96 ms with a re-scanned unsorted list).
// The list is sorted once at the end, so callers see the same ascending order (and summation order) as before.
constexpr int KNN_BLOCK = 64;
template <bool unused = true>
__device__ __forceinline__ int knn_query(const GridView &g, double qx, double qy, double qz, int k, double radius,
                                         double *sd /*[k][KNN_BLOCK] column tid*/, int *si) {
    const int t = threadIdx.x;
    const double r2 = radius > 0 ? radius * radius : 1e300;
    int cnt = 0;
    double maxd = 0.0;      // valid when cnt == k: the heap's root (the largest (d2, index) of the list)
    int maxslot = 0;
    const int cx = cell_coord(qx, g.ox, g.inv_cell), cy = cell_coord(qy, g.oy, g.inv_cell), cz = cell_coord(qz, g.oz, g.inv_cell);
    const int smax = max_shell(g, min(max(cx, 0), g.nx - 1), min(max(cy, 0), g.ny - 1), min(max(cz, 0), g.nz - 1)) + 1;
    // total order (d2, original index): exact-distance ties are common on voxelised / fp32-rounded clouds, and the oracle
    // breaks them the same way; the index loads stay off the hot path (only on an exact tie)
    auto greater = [&](double da, int sa, double db, int sb) {
        bool gt = da > db;
        if (da == db) gt = g.idx[sa] > g.idx[sb];
        return gt;
    };
    // puts (d2, i) at heap position pos and lets it sink to its place among the first n entries
    auto sift_down = [&](int pos, double d2, int i, int n) {
        for (;;) {
            int c = 2 * pos + 1;
            if (c >= n) break;
            double cd = sd[c * KNN_BLOCK + t];
            int cs = si[c * KNN_BLOCK + t];
            if (c + 1 < n) {
                const double rd = sd[(c + 1) * KNN_BLOCK + t];
                const int rs = si[(c + 1) * KNN_BLOCK + t];
                if (greater(rd, rs, cd, cs)) { c++; cd = rd; cs = rs; }
            }
            if (!greater(cd, cs, d2, i)) break;
            sd[pos * KNN_BLOCK + t] = cd;
            si[pos * KNN_BLOCK + t] = cs;
            pos = c;
        }
        sd[pos * KNN_BLOCK + t] = d2;
        si[pos * KNN_BLOCK + t] = i;
    };
    // candidates are fetched four at a time from clamped slots (no branch around a load)
    auto visit = [&](int b, int e) {
        for (int i0 = b; i0 < e; i0 += 4) {
            double X[4], Y[4], Z[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int64_t ii = min(i0 + u, e - 1);
                X[u] = g.pts[ii * 3]; Y[u] = g.pts[ii * 3 + 1]; Z[u] = g.pts[ii * 3 + 2];
            }
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int i = i0 + u;
                if (i >= e) break;
                const double dx = X[u] - qx, dy = Y[u] - qy, dz = Z[u] - qz;
                const double d2 = dx * dx + dy * dy + dz * dz;
                if (!(d2 < r2)) continue;
                if (cnt < k) {
                    sd[cnt * KNN_BLOCK + t] = d2;
                    si[cnt * KNN_BLOCK + t] = i;
                    if (++cnt == k) {                       // list full: make it a heap
                        for (int p = k / 2 - 1; p >= 0; p--) sift_down(p, sd[p * KNN_BLOCK + t], si[p * KNN_BLOCK + t], k);
                        maxd = sd[t]; maxslot = si[t];
                    }
                } else if (greater(maxd, maxslot, d2, i)) {
                    sift_down(0, d2, i, k);
                    maxd = sd[t]; maxslot = si[t];
                }
            }
        }
    };
    for (int s = 1; s <= smax; s++) {
        if (s == 1) for_block3(g, cx, cy, cz, visit);      // shells 0 and 1 as nine contiguous runs
        else for_shell_rows(g, qx, qy, qz, cx, cy, cz, s, [&]() { return cnt == k ? fmin(maxd, r2) : r2; }, visit);
        // everything not visited yet is at least s*cell away
        const double reach = s * g.cell;
        if (radius > 0 && reach >= radius) break;
        if (cnt == k && maxd <= reach * reach) break;
    }
    // ascending (d2, index): a full list is a heap, so heap-sort it in place (pop the maximum to the end, k - 1 times);
    // a list that never filled is in arrival order: heapify it first
    if (cnt < k)
        for (int p = cnt / 2 - 1; p >= 0; p--) sift_down(p, sd[p * KNN_BLOCK + t], si[p * KNN_BLOCK + t], cnt);
    for (int n = cnt - 1; n > 0; n--) {
        const double ld = sd[n * KNN_BLOCK + t], rd = sd[t];
        const int ls = si[n * KNN_BLOCK + t], rs = si[t];
        sd[n * KNN_BLOCK + t] = rd;
        si[n * KNN_BLOCK + t] = rs;
        sift_down(0, ld, ls, n);
    }
    return cnt;
}

// Normal of a neighbourhood covariance as legacy Open3D computes it: FastEigen3x3 [recalled: geometry/EstimateNormals.cpp, the
// closed form of geometrictools' RobustEigenSymmetric3x3] -- eigenvalues from the trigonometric solution of the characteristic
// cubic of A = cov / max coefficient, the eigenvector of the better-conditioned extreme eigenvalue from the largest cross product
// of two rows of A - lambda I, the middle one from the 2x2 problem in its orthogonal complement, the third as their cross
// product; returns the eigenvector of the smallest eigenvalue WITH THE SIGN THE FORMULAS PRODUCE (the reference's recorded
// normals carry exactly that sign).  The fused multiply-adds are placed explicitly (the library is built with
// -ffp-contract=off): they are the ones of the build that recorded the reference's frames, found by matching its 2.14 M recorded
// normals (oracle/normals.c header, profiles/r03_pin_normals.json: 89 % bit-equal sign included, all within 2e-12).  Cheaper
// than the cyclic Jacobi sweeps it replaces, and a degenerate neighbourhood now has the answer the original's formulas give.
__device__ __forceinline__ double fe_mulsub(double a, double b, double c, double d) { return fma(a, b, -(c * d)); }   // a*b - c*d
__device__ __forceinline__ void fe_cross(const double a[3], const double b[3], double o[3]) {
    o[0] = fe_mulsub(a[1], b[2], a[2], b[1]);
    o[1] = fe_mulsub(a[2], b[0], a[0], b[2]);
    o[2] = fe_mulsub(a[0], b[1], a[1], b[0]);
}
__device__ __forceinline__ void fe_eigenvector0(const double A[6], double ev, double o[3]) {
    const double r0[3] = {A[0] - ev, A[1], A[2]}, r1[3] = {A[1], A[3] - ev, A[4]}, r2[3] = {A[2], A[4], A[5] - ev};
    double c01[3], c02[3], c12[3];
    fe_cross(r0, r1, c01);
    fe_cross(r0, r2, c02);
    fe_cross(r1, r2, c12);
    const double d0 = fma(c01[2], c01[2], c01[0] * c01[0] + c01[1] * c01[1]);    // Eigen's 3-vector dot: packet of two + scalar tail
    const double d1 = fma(c02[2], c02[2], c02[0] * c02[0] + c02[1] * c02[1]);
    const double d2 = fma(c12[2], c12[2], c12[0] * c12[0] + c12[1] * c12[1]);
    // imax as the original: d1 replaces d0 if larger, d2 replaces the running maximum if larger (static selects only)
    const bool s1 = d1 > d0;
    const double dm = s1 ? d1 : d0;
    const bool s2 = d2 > dm;
    const double x = s2 ? c12[0] : (s1 ? c02[0] : c01[0]), y = s2 ? c12[1] : (s1 ? c02[1] : c01[1]), z = s2 ? c12[2] : (s1 ? c02[2] : c01[2]);
    const double l = sqrt(s2 ? d2 : dm);
    o[0] = x / l; o[1] = y / l; o[2] = z / l;
}
__device__ __forceinline__ void fe_eigenvector1(const double A[6], const double e0[3], double ev1, double o[3]) {
    double U[3], V[3];
    if (fabs(e0[0]) > fabs(e0[1])) {
        const double il = 1.0 / sqrt(fma(e0[0], e0[0], e0[2] * e0[2]));
        U[0] = -e0[2] * il; U[1] = 0.0; U[2] = e0[0] * il;
    } else {
        const double il = 1.0 / sqrt(fma(e0[1], e0[1], e0[2] * e0[2]));
        U[0] = 0.0; U[1] = e0[2] * il; U[2] = -e0[1] * il;
    }
    fe_cross(e0, U, V);
#define FE_SUM3(x0, y0, x1, y1, x2, y2) fma((x2), (y2), fma((x0), (y0), (x1) * (y1)))
    const double AU[3] = {FE_SUM3(A[0], U[0], A[1], U[1], A[2], U[2]), FE_SUM3(A[1], U[0], A[3], U[1], A[4], U[2]),
                          FE_SUM3(A[2], U[0], A[4], U[1], A[5], U[2])};
    const double AV[3] = {FE_SUM3(A[0], V[0], A[1], V[1], A[2], V[2]), FE_SUM3(A[1], V[0], A[3], V[1], A[4], V[2]),
                          FE_SUM3(A[2], V[0], A[4], V[1], A[5], V[2])};
    double m00 = FE_SUM3(U[0], AU[0], U[1], AU[1], U[2], AU[2]) - ev1;
    double m01 = FE_SUM3(U[0], AV[0], U[1], AV[1], U[2], AV[2]);
    double m11 = FE_SUM3(V[0], AV[0], V[1], AV[1], V[2], AV[2]) - ev1;
#undef FE_SUM3
    const double a00 = fabs(m00), a01 = fabs(m01), a11 = fabs(m11);
    double cu, cv;   // result = cu * U - cv * V
    if (a00 >= a11) {
        if (!(fmax(a00, a01) > 0)) { o[0] = U[0]; o[1] = U[1]; o[2] = U[2]; return; }
        if (a00 >= a01) { m01 /= m00; m00 = 1.0 / sqrt(fma(m01, m01, 1.0)); m01 *= m00; }
        else { m00 /= m01; m01 = 1.0 / sqrt(fma(m00, m00, 1.0)); m00 *= m01; }
        cu = m01; cv = m00;
    } else {
        if (!(fmax(a11, a01) > 0)) { o[0] = U[0]; o[1] = U[1]; o[2] = U[2]; return; }
        if (a11 >= a01) { m01 /= m11; m11 = 1.0 / sqrt(fma(m01, m01, 1.0)); m01 *= m11; }
        else { m11 /= m01; m01 = 1.0 / sqrt(fma(m11, m11, 1.0)); m11 *= m01; }
        cu = m11; cv = m01;
    }
#pragma unroll
    for (int i = 0; i < 3; i++) o[i] = fe_mulsub(cu, U[i], cv, V[i]);
}
// cov as c00 c01 c02 c11 c12 c22; n = (0,0,0) for an all-zero matrix (the caller substitutes (0,0,1) / the previous normal)
__device__ __forceinline__ void fast_eigen3x3(double c00, double c01, double c02, double c11, double c12, double c22, double n[3]) {
    const double mx = fmax(fmax(fmax(c00, c01), fmax(c02, c11)), fmax(c12, c22));
    n[0] = n[1] = n[2] = 0.0;
    if (mx == 0.0) return;
    const double A[6] = {c00 / mx, c01 / mx, c02 / mx, c11 / mx, c12 / mx, c22 / mx};
    const double norm = (A[1] * A[1] + A[2] * A[2]) + A[4] * A[4];
    if (!(norm > 0.0)) {   // diagonal matrix: the axis of the strictly smallest diagonal entry, z otherwise
        const double a00 = A[0] * mx, a11 = A[3] * mx, a22 = A[5] * mx;
        if (a00 < a11 && a00 < a22) n[0] = 1.0;
        else if (a11 < a00 && a11 < a22) n[1] = 1.0;
        else n[2] = 1.0;
        return;
    }
    const double q = (A[0] + A[3] + A[5]) / 3.0;
    const double b00 = A[0] - q, b11 = A[3] - q, b22 = A[5] - q;
    const double p = sqrt(fma(norm, 2.0, fma(b22, b22, fma(b00, b00, b11 * b11))) / 6.0);
    const double k00 = fe_mulsub(b11, b22, A[4], A[4]);
    const double k01 = fe_mulsub(A[1], b22, A[4], A[2]);
    const double k02 = fe_mulsub(A[1], A[4], b11, A[2]);
    const double det = fma(A[2], k02, fma(b00, k00, -(A[1] * k01))) / (p * p * p);
    const double half_det = fmin(fmax(det * 0.5, -1.0), 1.0);
    const double angle = acos(half_det) / 3.0;
    const double beta2 = cos(angle) * 2.0;
    const double beta0 = cos(angle + 2.09439510239319549) * 2.0;
    const double beta1 = -(beta0 + beta2);
    const double e0 = fma(p, beta0, q), e1 = fma(p, beta1, q), e2 = fma(p, beta2, q);
    double va[3], vb[3];
    if (half_det >= 0.0) {
        fe_eigenvector0(A, e2, va);                                    // evec2
        if (e2 < e0 && e2 < e1) { n[0] = va[0]; n[1] = va[1]; n[2] = va[2]; return; }
        fe_eigenvector1(A, va, e1, vb);                                // evec1
        if (e1 < e0 && e1 < e2) { n[0] = vb[0]; n[1] = vb[1]; n[2] = vb[2]; return; }
        fe_cross(vb, va, n);                                           // evec0 = evec1 x evec2
    } else {
        fe_eigenvector0(A, e0, va);                                    // evec0
        if (e0 < e1 && e0 < e2) { n[0] = va[0]; n[1] = va[1]; n[2] = va[2]; return; }
        fe_eigenvector1(A, va, e1, vb);                                // evec1
        if (e1 < e0 && e1 < e2) { n[0] = vb[0]; n[1] = vb[1]; n[2] = vb[2]; return; }
        fe_cross(va, vb, n);                                           // evec2 = evec0 x evec1
    }
}

// k_normals: one thread per (cell-sorted) point: hybrid / kNN search, population covariance, smallest eigenvector.
// < 3 neighbours -> (0,0,1).  If prev != NULL the sign follows the previous normal (legacy EstimateNormals).
__global__ void __launch_bounds__(KNN_BLOCK) k_normals(GridView g, int64_t n, int k, double radius, const double *__restrict__ prev,
                                                       double *__restrict__ normals, int *__restrict__ nn_count) {
    extern __shared__ double lds_d[];
    double *sd = lds_d;
    int *si = (int *)(lds_d + (size_t)k * KNN_BLOCK);
    int64_t i = (int64_t)blockIdx.x * KNN_BLOCK + threadIdx.x;
    if (i >= n) return;
    const int t = threadIdx.x;
    const double qx = g.pts[i * 3], qy = g.pts[i * 3 + 1], qz = g.pts[i * 3 + 2];
    const int cnt = knn_query(g, qx, qy, qz, k, radius, sd, si);
    // utility::ComputeCovariance [recalled]: ONE pass of nine cumulants over the RAW coordinates in neighbour order (nearest
    // first), products accumulated with fused multiply-adds, divided by the count, cov = E[ab] - E[a] E[b] (fused); fewer than
    // 3 neighbours: identity covariance, whose "normal" is (0,0,1).  Pinned by the recorded frames (oracle/normals.c).
    double nrm[3] = {0.0, 0.0, 0.0};
    if (cnt >= 3) {
        double sx = 0, sy = 0, sz = 0, xx = 0, xy = 0, xz = 0, yy = 0, yz = 0, zz = 0;
        for (int j0 = 0; j0 < cnt; j0 += 4) {       // four neighbours per round trip, summed in list order
            double X[4], Y[4], Z[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int64_t s = si[min(j0 + u, cnt - 1) * KNN_BLOCK + t];
                X[u] = g.pts[s * 3]; Y[u] = g.pts[s * 3 + 1]; Z[u] = g.pts[s * 3 + 2];
            }
#pragma unroll
            for (int u = 0; u < 4; u++) {
                if (j0 + u >= cnt) break;
                const double x = X[u], y = Y[u], z = Z[u];
                sx += x; sy += y; sz += z;
                xx = fma(x, x, xx); xy = fma(x, y, xy); xz = fma(x, z, xz); yy = fma(y, y, yy); yz = fma(y, z, yz); zz = fma(z, z, zz);
            }
        }
        const double dn = (double)cnt;
        sx /= dn; sy /= dn; sz /= dn; xx /= dn; xy /= dn; xz /= dn; yy /= dn; yz /= dn; zz /= dn;
        fast_eigen3x3(fma(-sx, sx, xx), fma(-sx, sy, xy), fma(-sx, sz, xz), fma(-sy, sy, yy), fma(-sy, sz, yz), fma(-sz, sz, zz), nrm);
    }
    const int64_t o = g.idx[i];
    const bool zero = nrm[0] == 0.0 && nrm[1] == 0.0 && nrm[2] == 0.0;     // < 3 neighbours or an all-zero covariance
    if (prev) {   // a cloud that already carries normals: a zero result keeps the old normal, every other one is turned towards it
        const double px = prev[o * 3], py = prev[o * 3 + 1], pz = prev[o * 3 + 2];
        if (zero) { nrm[0] = px; nrm[1] = py; nrm[2] = pz; }
        if ((nrm[0] * px + nrm[1] * py) + nrm[2] * pz < 0) { nrm[0] = -nrm[0]; nrm[1] = -nrm[1]; nrm[2] = -nrm[2]; }
    } else if (zero) nrm[2] = 1.0;
    normals[o * 3] = nrm[0]; normals[o * 3 + 1] = nrm[1]; normals[o * 3 + 2] = nrm[2];
    if (nn_count) nn_count[o] = cnt;
}

// k_knn_dist: mean of the k smallest distances (self included) -- statistical outlier removal's per-point score;
// with count_radius > 0 instead counts the neighbours within that radius (radius outlier removal)
__global__ void __launch_bounds__(KNN_BLOCK) k_knn_score(GridView g, int64_t n, int k, double count_radius, double *__restrict__ score) {
    extern __shared__ double lds_d[];
    double *sd = lds_d;
    int *si = (int *)(lds_d + (size_t)k * KNN_BLOCK);
    int64_t i = (int64_t)blockIdx.x * KNN_BLOCK + threadIdx.x;
    if (i >= n) return;
    const int t = threadIdx.x;
    const double qx = g.pts[i * 3], qy = g.pts[i * 3 + 1], qz = g.pts[i * 3 + 2];
    if (count_radius > 0) {
        const double r2 = count_radius * count_radius;
        const int cx = cell_coord(qx, g.ox, g.inv_cell), cy = cell_coord(qy, g.oy, g.inv_cell), cz = cell_coord(qz, g.oz, g.inv_cell);
        int c = 0;
        const int smax = (int)ceil(count_radius * g.inv_cell);
        auto count = [&](int b, int e) {
            for (int j = b; j < e; j++) {
                double dx = g.pts[(int64_t)j * 3] - qx, dy = g.pts[(int64_t)j * 3 + 1] - qy, dz = g.pts[(int64_t)j * 3 + 2] - qz;
                if (dx * dx + dy * dy + dz * dz <= r2) c++;
            }
        };
        for_block3(g, cx, cy, cz, count);
        for (int s = 2; s <= smax; s++) for_shell(g, cx, cy, cz, s, count);
        score[g.idx[i]] = (double)c;
        return;
    }
    const int cnt = knn_query(g, qx, qy, qz, k, -1.0, sd, si);
    double a = 0;
    for (int j = 0; j < cnt; j++) a += sqrt(sd[j * KNN_BLOCK + t]);
    score[g.idx[i]] = cnt ? a / cnt : 0.0;
}

// k_knn_graph: indices (original numbering) and squared distances of the k nearest points, nearest first
// (the point itself comes first); rows shorter than k are padded with -1 / +inf
__global__ void __launch_bounds__(KNN_BLOCK) k_knn_graph(GridView g, int64_t n, int k, double radius, int *__restrict__ nbr,
                                                         double *__restrict__ d2) {
    extern __shared__ double lds_d[];
    double *sd = lds_d;
    int *si = (int *)(lds_d + (size_t)k * KNN_BLOCK);
    int64_t i = (int64_t)blockIdx.x * KNN_BLOCK + threadIdx.x;
    if (i >= n) return;
    const int t = threadIdx.x;
    const int cnt = knn_query(g, g.pts[i * 3], g.pts[i * 3 + 1], g.pts[i * 3 + 2], k, radius, sd, si);
    const int64_t o = g.idx[i];
    for (int j = 0; j < k; j++) {
        nbr[o * k + j] = j < cnt ? g.idx[si[j * KNN_BLOCK + t]] : -1;
        if (d2) d2[o * k + j] = j < cnt ? sd[j * KNN_BLOCK + t] : 1e300;
    }
}

// ------------------------------------------------------------------------------------------------ ICP
// One launch = one "GetRegistrationResultAndCorrespondences" + the sums the NEXT ComputeTransformation needs:
// for every source point p = T s: nearest target point within max_dist (strict <), then
//   slots [0] n  [1] sum d^2
//   P2P    : [2..4] sum p, [5..7] sum t, [8..16] sum p t^T (row-major p_i t_j)
//   P2PLANE: [2..22] upper triangle of J^T J (J = [p x n_t ; n_t]), [23..28] J^T r, r = (p - t).n_t
//   GICP   : same slots with J^T J = Jb^T M^-1 Jb, J^T r = Jb^T M^-1 d, Jb = [-[p]x | I], d = p - t,
//            M = C_t + R C_s R^T with C = I - (1-eps) n n^T   (== W^T W with W = M^-1/2 of the original)
//   COLORED: the P2PLANE slots over TWO rows per correspondence (Open3D ColoredICP.cpp ComputeTransformation [recalled]):
//            e = (p - t).n_t;  J_G = sg [p x n_t ; n_t], r_G = sg e;  with d_t / I_t the target's intensity gradient / intensity,
//            I_s the source intensity, p' = p - e n_t:  m = -(d_t - (d_t.n_t) n_t),  J_I = sp [p x m ; m],
//            r_I = sp (I_s - (d_t.(p' - t) + I_t));  sg = sqrt(lambda), sp = sqrt(1 - lambda)
constexpr int ICP_SLOTS = 29;
constexpr int ICP_BLOCK = 256;
enum { MODE_P2P = 0, MODE_P2PLANE = 1, MODE_GICP = 2, MODE_COLORED = 3 };
// what the coloured mode reads besides the point-to-plane inputs; passed by value behind the other kernel arguments (unused, and
// zero, in every other mode)
struct IcpColor {
    const double *src_i;    // [ns] source intensity, in the order of the (Morton-sorted) source
    const double *tgt_ig;   // [nt][4] target intensity + gradient (k_color_gradient's record), cell-sorted
    double sg, sp;          // sqrt(lambda), sqrt(1 - lambda)
};

struct Rigid { double r[9], t[3]; };
// p = T s as the registration forms it: ((r0 sx + r1 sy) + r2 sz) + t per row
__device__ __forceinline__ void rigid_apply(const Rigid &T, double sx, double sy, double sz, double &px, double &py, double &pz) {
    px = T.r[0] * sx + T.r[1] * sy + T.r[2] * sz + T.t[0];
    py = T.r[3] * sx + T.r[4] * sy + T.r[5] * sz + T.t[1];
    pz = T.r[6] * sx + T.r[7] * sy + T.r[8] * sz + T.t[2];
}
// the point the point-to-point slots are relative to: the centre of the target grid's box (icp_setup)
struct IcpOrigin { double x, y, z; };

// Device-resident state of one registration loop: the evaluation kernels read the pose from here and k_icp_step advances it,
// so consecutive iterations are enqueued back to back without a host round trip (the host looks at `done` once per batch).
struct IcpState {
    double T[16];             // pose used by the next evaluation (row-major 4x4)
    double fit, rmse, corr;   // statistics of the latest evaluation
    int evals;                // evaluations consumed so far
    int done, converged, iterations;
    // device clock (wall_clock64, 100 MHz) at the first and the latest step: the GPU-side duration of the loop, to tell a stall
    // of the device from a completion that reached the host late (R3D_ICP_DEBUG=1 prints both when they disagree)
    unsigned long long t_first, t_last;
    int seq;                  // host mirror only: evaluations published so far (written LAST, after a system-scope fence)
};
constexpr int ICP_SEQ_DONE = 1 << 30;   // bit of the mirror's `seq` word: the loop has ended (published with the sequence number)
__device__ __forceinline__ Rigid load_rigid(const IcpState *__restrict__ st) {
    Rigid T;
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) T.r[i * 3 + j] = st->T[i * 4 + j];
        T.t[i] = st->T[i * 4 + 3];
    }
    return T;
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

__device__ __forceinline__ bool inv3_sym(const double m[6] /*xx xy xz yy yz zz*/, double a[6]) {
    const double c00 = m[3] * m[5] - m[4] * m[4], c01 = m[2] * m[4] - m[1] * m[5], c02 = m[1] * m[4] - m[2] * m[3];
    const double det = m[0] * c00 + m[1] * c01 + m[2] * c02;
    if (fabs(det) < 1e-300) return false;
    const double id = 1.0 / det;
    a[0] = c00 * id; a[1] = c01 * id; a[2] = c02 * id;
    a[3] = (m[0] * m[5] - m[2] * m[2]) * id; a[4] = (m[1] * m[2] - m[0] * m[4]) * id; a[5] = (m[0] * m[3] - m[1] * m[1]) * id;
    return true;
}

// ---- coloured ICP set-up (Open3D ColoredICP.cpp InitializePointCloudForColoredICP [recalled]; contract in DESIGN.md section 4, "Coloured ICP")
// intensity I = (r + g + b) / 3 of point idx[i] (idx null: point i), summed in that order
__global__ void __launch_bounds__(256) k_intensity(const double *__restrict__ colors, const int *__restrict__ idx, int64_t n, double *__restrict__ out) {
    int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t j = idx ? idx[i] : i;
    out[i] = ((colors[j * 3] + colors[j * 3 + 1]) + colors[j * 3 + 2]) / 3.0;
}

__global__ void __launch_bounds__(256) k_gather4(const double *__restrict__ src, const int *__restrict__ idx, int64_t n, double *__restrict__ dst) {
    int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t j = idx[i];
    dst[i * 4] = src[j * 4]; dst[i * 4 + 1] = src[j * 4 + 1]; dst[i * 4 + 2] = src[j * 4 + 2]; dst[i * 4 + 3] = src[j * 4 + 3];
}

// k_color_gradient: one thread per (cell-sorted) point: the hybrid search of k_normals, then the least-squares intensity gradient
// in the point's tangent plane.  Neighbour i >= 1 (the list's first entry is the point itself) contributes the row
// a_i = (p_i - ((p_i - v).n) n) - v with right-hand side I_i - I_v, a last row (nn - 1) n with right-hand side 0 keeps the
// gradient out of the normal direction; the 3x3 normal equations are summed in list order and solved with inv3_sym.  Fewer than
// 4 neighbours, a singular system or a non-finite solution give a zero gradient (QUIRK_SINGULAR: the original's LDLT result is
// unspecified there).  rec (the caller's numbering): [4 o] = intensity, [4 o + 1 .. 3] = gradient.
__global__ void __launch_bounds__(KNN_BLOCK) k_color_gradient(GridView g, int64_t n, int k, double radius, const double *__restrict__ normals /* caller's numbering */,
                                                              const double *__restrict__ inten /* cell-sorted */, double *__restrict__ rec) {
    extern __shared__ double lds_d[];
    double *sd = lds_d;
    int *si = (int *)(lds_d + (size_t)k * KNN_BLOCK);
    int64_t i = (int64_t)blockIdx.x * KNN_BLOCK + threadIdx.x;
    if (i >= n) return;
    const int t = threadIdx.x;
    const double qx = g.pts[i * 3], qy = g.pts[i * 3 + 1], qz = g.pts[i * 3 + 2];
    const int cnt = knn_query(g, qx, qy, qz, k, radius, sd, si);
    const int64_t o = g.idx[i];
    const double it = inten[i];
    double grad[3] = {0.0, 0.0, 0.0};
    if (cnt >= 4) {
        const double nx = normals[o * 3], ny = normals[o * 3 + 1], nz = normals[o * 3 + 2];
        double m[6] = {0, 0, 0, 0, 0, 0}, bx = 0, by = 0, bz = 0;
        for (int j0 = 1; j0 < cnt; j0 += 4) {       // four neighbours per round trip, summed in list order
            double X[4], Y[4], Z[4], I[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int64_t s = si[min(j0 + u, cnt - 1) * KNN_BLOCK + t];
                X[u] = g.pts[s * 3]; Y[u] = g.pts[s * 3 + 1]; Z[u] = g.pts[s * 3 + 2];
                I[u] = inten[s];
            }
#pragma unroll
            for (int u = 0; u < 4; u++) {
                if (j0 + u >= cnt) break;
                const double dot = ((X[u] - qx) * nx + (Y[u] - qy) * ny) + (Z[u] - qz) * nz;
                const double ax = (X[u] - dot * nx) - qx, ay = (Y[u] - dot * ny) - qy, az = (Z[u] - dot * nz) - qz;
                const double b = I[u] - it;
                m[0] += ax * ax; m[1] += ax * ay; m[2] += ax * az; m[3] += ay * ay; m[4] += ay * az; m[5] += az * az;
                bx += ax * b; by += ay * b; bz += az * b;
            }
        }
        const double w = (double)(cnt - 1);
        const double lx = w * nx, ly = w * ny, lz = w * nz;
        m[0] += lx * lx; m[1] += lx * ly; m[2] += lx * lz; m[3] += ly * ly; m[4] += ly * lz; m[5] += lz * lz;
        double a[6];
        if (inv3_sym(m, a)) {
            const double gx = (a[0] * bx + a[1] * by) + a[2] * bz, gy = (a[1] * bx + a[3] * by) + a[4] * bz, gz = (a[2] * bx + a[4] * by) + a[5] * bz;
            if (isfinite(gx) && isfinite(gy) && isfinite(gz)) { grad[0] = gx; grad[1] = gy; grad[2] = gz; }
        }
    }
    rec[o * 4] = it; rec[o * 4 + 1] = grad[0]; rec[o * 4 + 2] = grad[1]; rec[o * 4 + 3] = grad[2];
}

// ------------------------------------------------------------------------------------------------ FPFH
// Open3D pipelines/registration/Feature.cpp [recalled]; the contract is restated in DESIGN.md section 4 ("FPFH") and, executable,
// in tests/fpfh_ref.py.  All arithmetic is float64 in the order written there (the build has -ffp-contract=off); only acos and
// atan2 come from the device's libm, and where their last bit could decide a bin or the role swap the restatement says so.
constexpr int FPFH_DIM = 33;
constexpr double FPFH_PI = 3.14159265358979323846;

// the search's lists of one thread, LDS columns -> global [slot][n] columns (coalesced over the wave) for k_fpfh
__device__ __forceinline__ void fpfh_store_lists(const double *sd, const int *si, int t, int64_t i, int64_t n, int cnt, int *__restrict__ l_cnt,
                                                 int *__restrict__ l_idx, double *__restrict__ l_d2) {
    l_cnt[i] = cnt;
    for (int j = 1; j < cnt; j++) {
        l_idx[(int64_t)(j - 1) * n + i] = si[j * KNN_BLOCK + t];      // slot 0 (the point itself) is not stored
        l_d2[(int64_t)(j - 1) * n + i] = sd[j * KNN_BLOCK + t];
    }
}

// pair feature of (p1, n1) and (p2, n2): f[0] = atan2 angle, f[1] = v . n2', f[2] = +-cos of the better-aligned normal
__device__ __forceinline__ void fpfh_pair(double p1x, double p1y, double p1z, double n1x, double n1y, double n1z, double p2x, double p2y, double p2z,
                                          double n2x, double n2y, double n2z, double f[3]) {
    f[0] = f[1] = f[2] = 0.0;
    double dx = p2x - p1x, dy = p2y - p1y, dz = p2z - p1z;
    const double f3 = sqrt((dx * dx + dy * dy) + dz * dz);
    if (f3 == 0.0) return;
    const double a1 = ((n1x * dx + n1y * dy) + n1z * dz) / f3, a2 = ((n2x * dx + n2y * dy) + n2z * dz) / f3;
    const bool swap = acos(fabs(a1)) > acos(fabs(a2));
    const double ax = swap ? n2x : n1x, ay = swap ? n2y : n1y, az = swap ? n2z : n1z;    // n1'
    const double bx = swap ? n1x : n2x, by = swap ? n1y : n2y, bz = swap ? n1z : n2z;    // n2'
    if (swap) { dx = -dx; dy = -dy; dz = -dz; }
    double vx = dy * az - dz * ay, vy = dz * ax - dx * az, vz = dx * ay - dy * ax;       // dp x n1'
    const double vn = sqrt((vx * vx + vy * vy) + vz * vz);
    if (vn == 0.0) return;
    vx /= vn; vy /= vn; vz /= vn;
    const double wx = ay * vz - az * vy, wy = az * vx - ax * vz, wz = ax * vy - ay * vx; // n1' x v
    f[2] = swap ? -a2 : a1;
    f[1] = (vx * bx + vy * by) + vz * bz;
    f[0] = atan2((wx * bx + wy * by) + wz * bz, (ax * bx + ay * by) + az * bz);
}
__device__ __forceinline__ int fpfh_bin(double c) {   // floor, clamped to the group's 11 bins (NaN -> 0, as a failed int conversion clamps)
    const double fl = floor(c);
    return fl >= 10.0 ? 10 : (fl >= 1.0 ? (int)fl : 0);
}

// k_spfh: one thread per (cell-sorted) point: the hybrid search of k_normals, the lists stored for k_fpfh, then the simplified
// histogram.  Every increment of one point is the same h = 100 / (nn - 1), so the 33 bins are COUNTED (<= 127 each) in 8-bit
// fields of nine registers -- three per group of 11 bins, selected with static indices -- and multiplied by h at the end; a
// dynamically indexed double[33] would live in scratch.  Rows go out in cell-sorted order (spfh_s, what k_fpfh gathers from:
// neighbours are near each other there) and, if asked for, in the caller's numbering.
__global__ void __launch_bounds__(KNN_BLOCK) k_spfh(GridView g, int64_t n, int k, double radius, const double *__restrict__ nrm_s /* cell-sorted */,
                                                    int *__restrict__ l_cnt, int *__restrict__ l_idx, double *__restrict__ l_d2,
                                                    double *__restrict__ spfh_s, double *__restrict__ spfh_o /* caller's numbering, or null */) {
    extern __shared__ double lds_d[];
    double *sd = lds_d;
    int *si = (int *)(lds_d + (size_t)k * KNN_BLOCK);
    int64_t i = (int64_t)blockIdx.x * KNN_BLOCK + threadIdx.x;
    if (i >= n) return;
    const int t = threadIdx.x;
    const double qx = g.pts[i * 3], qy = g.pts[i * 3 + 1], qz = g.pts[i * 3 + 2];
    const int cnt = knn_query(g, qx, qy, qz, k, radius, sd, si);
    fpfh_store_lists(sd, si, t, i, n, cnt, l_cnt, l_idx, l_d2);
    const double nx = nrm_s[i * 3], ny = nrm_s[i * 3 + 1], nz = nrm_s[i * 3 + 2];
    unsigned c[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int j0 = 1; j0 < cnt; j0 += 2) {       // two neighbours per round trip
        double P[2][3], N[2][3];
#pragma unroll
        for (int u = 0; u < 2; u++) {
            const int64_t s = si[min(j0 + u, cnt - 1) * KNN_BLOCK + t];
#pragma unroll
            for (int a = 0; a < 3; a++) { P[u][a] = g.pts[s * 3 + a]; N[u][a] = nrm_s[s * 3 + a]; }
        }
#pragma unroll
        for (int u = 0; u < 2; u++) {
            if (j0 + u >= cnt) break;
            double f[3];
            fpfh_pair(qx, qy, qz, nx, ny, nz, P[u][0], P[u][1], P[u][2], N[u][0], N[u][1], N[u][2], f);
            const int b[3] = {fpfh_bin(11.0 * (f[0] + FPFH_PI) / (2.0 * FPFH_PI)), fpfh_bin(11.0 * (f[1] + 1.0) * 0.5),
                              fpfh_bin(11.0 * (f[2] + 1.0) * 0.5)};
#pragma unroll
            for (int gq = 0; gq < 3; gq++) {
                const unsigned one = 1u << ((b[gq] & 3) * 8);
                const int w = b[gq] >> 2;
#pragma unroll
                for (int q = 0; q < 3; q++) c[gq * 3 + q] += w == q ? one : 0u;
            }
        }
    }
    const double h = cnt > 1 ? 100.0 / (double)(cnt - 1) : 0.0;
    const int64_t o = g.idx[i];
#pragma unroll
    for (int j = 0; j < FPFH_DIM; j++) {
        const int gq = j / 11, b = j % 11;
        const double v = (double)((c[gq * 3 + (b >> 2)] >> ((b & 3) * 8)) & 255u) * h;
        spfh_s[i * FPFH_DIM + j] = v;
        if (spfh_o) spfh_o[o * FPFH_DIM + j] = v;
    }
}

// the search and the stored lists alone (r3d_fpfh_from_spfh: the second stage on a caller-supplied SPFH)
__global__ void __launch_bounds__(KNN_BLOCK) k_fpfh_lists(GridView g, int64_t n, int k, double radius, int *__restrict__ l_cnt, int *__restrict__ l_idx,
                                                          double *__restrict__ l_d2) {
    extern __shared__ double lds_d[];
    double *sd = lds_d;
    int *si = (int *)(lds_d + (size_t)k * KNN_BLOCK);
    int64_t i = (int64_t)blockIdx.x * KNN_BLOCK + threadIdx.x;
    if (i >= n) return;
    const int cnt = knn_query(g, g.pts[i * 3], g.pts[i * 3 + 1], g.pts[i * 3 + 2], k, radius, sd, si);
    fpfh_store_lists(sd, si, threadIdx.x, i, n, cnt, l_cnt, l_idx, l_d2);
}

// rows of 33 doubles from the caller's numbering into cell-sorted order
__global__ void __launch_bounds__(256) k_gather_rows33(const double *__restrict__ src, const int *__restrict__ idx, int64_t n, double *__restrict__ dst) {
    int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n * FPFH_DIM) return;
    const int64_t i = e / FPFH_DIM;
    dst[e] = src[(int64_t)idx[i] * FPFH_DIM + (e - i * FPFH_DIM)];
}

// k_fpfh: one thread per (cell-sorted) point: the SPFH rows of its neighbours (list order, the point itself and coincident
// points skipped) weighted by 1 / d2, each group of 11 scaled to 100, plus the point's own row.  33 + 3 accumulators with
// static indices; the lists are k_spfh's ([slot][n]: a wave reads a slot of 64 consecutive points as one run).
__global__ void __launch_bounds__(64) k_fpfh(int64_t n, const int *__restrict__ l_cnt, const int *__restrict__ l_idx, const double *__restrict__ l_d2,
                                             const double *__restrict__ spfh_s, const int *__restrict__ idx, double *__restrict__ fpfh) {
    int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const int cnt = l_cnt[i];
    double f[FPFH_DIM], sum[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int j = 0; j < FPFH_DIM; j++) f[j] = 0.0;
    for (int q = 1; q < cnt; q++) {
        const double d2 = l_d2[(int64_t)(q - 1) * n + i];
        const double *__restrict__ row = spfh_s + (int64_t)l_idx[(int64_t)(q - 1) * n + i] * FPFH_DIM;
        if (d2 == 0.0) continue;
#pragma unroll
        for (int j = 0; j < FPFH_DIM; j++) {
            const double val = row[j] / d2;
            sum[j / 11] += val;
            f[j] += val;
        }
    }
#pragma unroll
    for (int gq = 0; gq < 3; gq++) if (sum[gq] != 0.0) sum[gq] = 100.0 / sum[gq];
    const double *__restrict__ own = spfh_s + i * FPFH_DIM;
    double *__restrict__ out = fpfh + (int64_t)idx[i] * FPFH_DIM;
#pragma unroll
    for (int j = 0; j < FPFH_DIM; j++) out[j] = f[j] * sum[j / 11] + own[j];
}

// k_match_features: nearest target row of every source row under (sum_j (a_j - b_j)^2 in j order, target index), brute force in
// float64.  One source row per thread in registers; the targets of this block's share (blockIdx.y of gridDim.y equal runs of
// tiles) are staged MATCH_TILE rows at a time in LDS and read by every lane at the same address (a broadcast).  Strict < keeps
// the smaller index inside a share; k_match_reduce folds the shares in ascending target order with the same rule.
constexpr int MATCH_TILE = 128, MATCH_BLOCK = 256;
__global__ void __launch_bounds__(MATCH_BLOCK) k_match_features(const double *__restrict__ src, int64_t ns, const double *__restrict__ tgt, int64_t nt,
                                                               int64_t tiles_per_share, double *__restrict__ part_d2, int *__restrict__ part_idx) {
    __shared__ double tile[MATCH_TILE * FPFH_DIM];
    const int64_t i = (int64_t)blockIdx.x * MATCH_BLOCK + threadIdx.x;
    const int64_t ic = i < ns ? i : ns - 1;     // a lane past the end works on the last row (it takes part in the staging) and writes nothing
    double a[FPFH_DIM];
#pragma unroll
    for (int j = 0; j < FPFH_DIM; j++) a[j] = src[ic * FPFH_DIM + j];
    double best = __builtin_huge_val();         // +inf: any finite distance beats it
    int bi = -1;
    const int64_t t0 = (int64_t)blockIdx.y * tiles_per_share * MATCH_TILE;
    const int64_t t1 = t0 + tiles_per_share * MATCH_TILE < nt ? t0 + tiles_per_share * MATCH_TILE : nt;
    for (int64_t tb = t0; tb < t1; tb += MATCH_TILE) {
        const int rows = (int)(t1 - tb < MATCH_TILE ? t1 - tb : MATCH_TILE);
        __syncthreads();
        for (int e = threadIdx.x; e < rows * FPFH_DIM; e += MATCH_BLOCK) tile[e] = tgt[tb * FPFH_DIM + e];
        __syncthreads();
        for (int r = 0; r < rows; r++) {
            const double *__restrict__ b = tile + r * FPFH_DIM;
            double acc = 0.0;
#pragma unroll
            for (int j = 0; j < FPFH_DIM; j++) { const double d = a[j] - b[j]; acc += d * d; }
            if (acc < best) { best = acc; bi = (int)(tb + r); }
        }
    }
    if (i < ns) { part_d2[(int64_t)blockIdx.y * ns + i] = best; part_idx[(int64_t)blockIdx.y * ns + i] = bi; }
}
__global__ void __launch_bounds__(256) k_match_reduce(const double *__restrict__ part_d2, const int *__restrict__ part_idx, int64_t ns, int shares,
                                                      int *__restrict__ nn, double *__restrict__ d2) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= ns) return;
    double best = part_d2[i];
    int bi = part_idx[i];
    for (int s = 1; s < shares; s++) {
        const double d = part_d2[(int64_t)s * ns + i];
        const int q = part_idx[(int64_t)s * ns + i];
        if (q >= 0 && (bi < 0 || d < best)) { best = d; bi = q; }
    }
    nn[i] = bi;
    if (d2) d2[i] = best;
}

// nearest target point inside the 3x3x3 cell block around the query (shells 0 and 1), straight from global memory, as nine
// contiguous runs.  All 18 run bounds are requested before any is used, and the candidates of a run are fetched four at a
// time (clamped index, no branch around a load): the search is a chain of dependent gathers otherwise.
__device__ __forceinline__ void nn_block_global(const GridView &g, double px, double py, double pz, int cx, int cy, int cz, double &best,
                                                int &bi) {
    const int xa = cx - 1, xb = cx + 1;
    const bool xok = xb >= 0 && xa <= g.nx - 1;
    const int x0 = min(max(xa, 0), g.nx - 1), x1 = min(max(xb, 0), g.nx - 1);
    int rb[9], re[9];
#pragma unroll
    for (int r = 0; r < 9; r++) {
        const int z = cz + r / 3 - 1, y = cy + r % 3 - 1;
        const bool ok = xok && z >= 0 && z < g.nz && y >= 0 && y < g.ny;
        const int64_t row = ((int64_t)min(max(z, 0), g.nz - 1) * g.ny + min(max(y, 0), g.ny - 1)) * g.nx;
        // both bounds of the run with ONE 16-byte request (the end entry is at most three behind the start entry; the table
        // is allocated with four spare entries); the search is bound by the number of cache-line requests, not by latency
        const cs_int4 cs = cs4(g, row + x0);
        const int b = cs.x, de = x1 + 1 - x0, e = de == 3 ? cs.w : de == 2 ? cs.z : cs.y;
        rb[r] = b;
        re[r] = b + ((e - b) & (ok ? -1 : 0));
    }
#pragma unroll
    for (int r = 0; r < 9; r++) {
        const int e = re[r];
        for (int j0 = rb[r]; j0 < e; j0 += 4) {
            double X[4], Y[4], Z[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int64_t jj = min(j0 + u, e - 1);
                X[u] = g.pts[jj * 3]; Y[u] = g.pts[jj * 3 + 1]; Z[u] = g.pts[jj * 3 + 2];
            }
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int j = j0 + u;
                const double dx = X[u] - px, dy = Y[u] - py, dz = Z[u] - pz;
                const double d2 = dx * dx + dy * dy + dz * dz;
                if (j < e && d2 <= best) {  // ties are rare: the index loads of the total order (d2, index) stay off the hot path
                    if (d2 < best || (bi >= 0 && g.idx[j] < g.idx[bi])) { best = d2; bi = j; }
                }
            }
        }
    }
}

// Two-stage, packed form of the same search (the default).  The all-float64 loop is bound by the texture-addresser / L1 path
// (a float64 candidate costs two gather instructions, 24 bytes = dwordx4 + dwordx2), and a float32 scan that keeps (distance,
// slot) pairs is bound by the vector ALU: 37 instructions per candidate, most of them the sorted insertion into a quadruple,
// every one of the nine rows walked by the whole wave for as long as its longest lane.  Here STAGE 1 scans a packed copy of
// the candidates and keeps the four smallest approximate distances, branch-free, and STAGE 2 evaluates the best three exactly
// (float64, the update rule and tie order of nn_block_global).  With |d_stage1 - d_exact| <= FEQ / 2 for every candidate,
// every candidate that can be the exact nearest point, or tie with it, has a stage-1 distance within FEQ of the smallest one;
// if the FOURTH smallest is within that margin too, the three may not contain them all and the lane falls back to
// nn_block_global (rare: four candidates within a fraction of a cell of the same distance).  In stage 1
//  (1) a candidate is ONE dword: its position inside its own cell quantised to 10 bits per axis, x together with the low two
//      bits of its cell x index (k_pack_q10): one 16-byte gather brings four candidates, and the query is expressed in the
//      same unit (cell / 1024) relative to the corner of its 3x3x3 block, where every coordinate is below 4096 and float32
//      is exact to 2^-11 units;
//  (2) distance and candidate travel as ONE 32-bit key: the float bits of the squared distance with the low 10 mantissa
//      bits replaced by the candidate's ordinal in this query's scan, so the sorted insertion into the best four is
//      v_min + 3 x v_med3 (20 instructions per candidate in all);
//  (3) the centre row is scanned first; a row whose slab distance to the query exceeds the margin threshold of the best
//      distance so far (or the correspondence radius) is dropped: it cannot hold the nearest point, a tie with it, or a
//      contender that the fallback test would have to count; the surviving rows go to a per-lane list (LDS, column per
//      thread) that is walked in ONE loop, so a wave iterates max-over-lanes of the per-lane total instead of the sum over
//      rows of the per-row maximum.
// Error budget of stage 1 in units: reconstruction of a candidate 0.5 per axis (0.867 in distance), the query's float
// coordinates 2.5e-4, key truncation 2^-13 relative in d^2 (<= 0.22 at the far corner of the block): |d_stage1 - d_exact| <=
// 1.1, so the margin FEQ = 2.25 units = cell / 455.  The result is bit-identical to the all-float64 search
// (tests/test_cloud_gpu.py).  Queries whose nine rows hold more than 1024 candidates use the fallback.
constexpr float FEQ = 2.25f;
// pooled walk (nn_block_q10<1>): queue capacity per wave, and words per wave of the pool buffer: keys [Q][4], items [Q][2], the
// lanes' query parameters [4][64], the queue length
constexpr int POOL_Q = 256;
constexpr int pool_words(int q) { return 6 * q + 256 + 4; }

__global__ void __launch_bounds__(256) k_pack_q10(GridView g, int64_t n, unsigned *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n + 4) return;
    unsigned w = 0;
    if (i < n) {
        const double u[3] = {(g.pts[i * 3] - g.ox) * g.inv_cell, (g.pts[i * 3 + 1] - g.oy) * g.inv_cell, (g.pts[i * 3 + 2] - g.oz) * g.inv_cell};
        const int dims[3] = {g.nx, g.ny, g.nz};
        unsigned q[3];
        int c0 = 0;
#pragma unroll
        for (int a = 0; a < 3; a++) {
            const int c = min(max((int)floor(u[a]), 0), dims[a] - 1);   // the cell the point was sorted into (k_cell_keys)
            q[a] = (unsigned)min(max((int)floor((u[a] - c) * 1024.0), 0), 1023);
            if (a == 0) c0 = c;
        }
        w = q[0] | (unsigned)(c0 & 3) << 10 | q[1] << 12 | q[2] << 22;
    }
    out[i] = w;
}

__device__ __forceinline__ int med3_i32(int a, int b, int c) { return max(min(a, b), min(max(a, b), c)); }

// G: groups of four candidates requested together before any of them is used (1: one gather per step of the scan, the form for
// large clouds, where three waves per SIMD hide the gathers; 3: for clouds so small that a SIMD holds one wave -- a scanning-loop
// frame of 40 k points is 160 workgroups on 256 CUs -- and every dependent gather is a full memory round trip: the same candidates
// in the same order, so the same keys and the same result)
template <int G>
__device__ __forceinline__ void nn_block_q10(const GridView &g, double px, double py, double pz, int cx, int cy, int cz, double r2,
                                             double &best, int &bi, int *__restrict__ sRun /* [18][ICP_BLOCK] */,
                                             int *__restrict__ sPool = nullptr /* G == 1: [ICP_BLOCK / 64][pool_words(POOL_Q)], 16-byte aligned */) {
    constexpr int B = 256;   // = ICP_BLOCK (declared below)
    const int tid = threadIdx.x;
    const int xa = cx - 1, xb = cx + 1;
    const bool xok = xb >= 0 && xa <= g.nx - 1;
    const int x0 = min(max(xa, 0), g.nx - 1), x1 = min(max(xb, 0), g.nx - 1);
    typedef unsigned uint4_a4 __attribute__((ext_vector_type(4), aligned(4)));
    constexpr int ORD[9] = {4, 1, 3, 5, 7, 0, 2, 6, 8};   // centre row, the four rows sharing a face with it, the four corners
    int rb[9], re[9], rm1[9], rm2[9], total = 0;   // run bounds and the two cell boundaries inside a full three-cell run
    // table index of the run's first cell: the table has at most 2^26 entries (grid_build), so 32-bit arithmetic, two vector
    // multiplies for all nine rows (the row offsets are wave-uniform); rows outside the grid read entry 0 and are emptied
    const unsigned base = ((unsigned)(cz - 1) * (unsigned)g.ny + (unsigned)(cy - 1)) * (unsigned)g.nx + (unsigned)x0;
    const int de = x1 + 1 - x0;
#pragma unroll
    for (int q = 0; q < 9; q++) {
        const int r = ORD[q], rz = r / 3, ry = r % 3;
        const bool ok = xok && (unsigned)(cz + rz - 1) < (unsigned)g.nz && (unsigned)(cy + ry - 1) < (unsigned)g.ny;
        const unsigned off = ((unsigned)rz * (unsigned)g.ny + (unsigned)ry) * (unsigned)g.nx;
        const cs_int4 cs = cs4(g, (int64_t)(ok ? base + off : 0u));
        const int b = cs.x, e = de == 3 ? cs.w : de == 2 ? cs.z : cs.y;
        rb[q] = b;
        re[q] = b + ((e - b) & (ok ? -1 : 0));
        rm1[q] = cs.y;
        rm2[q] = cs.z;
        total += (re[q] - rb[q] + 3) & ~3;
    }
    if (total > 1024) {                            // the ordinal field of the keys would overflow (very dense cells)
        nn_block_global(g, px, py, pz, cx, cy, cz, best, bi);
        return;
    }
    // the query in units of cell / 1024 relative to the block corner (cx-1, cy-1, cz-1): [1024, 2048) on every axis
    const double ux = (px - g.ox) * g.inv_cell, uy = (py - g.oy) * g.inv_cell, uz = (pz - g.oz) * g.inv_cell;
    const float qxc = (float)((ux - (double)(cx - 1)) * 1024.0), qyc = (float)((uy - (double)(cy - 1)) * 1024.0),
                qzc = (float)((uz - (double)(cz - 1)) * 1024.0);
    const float qx = qxc - 0.5f;                   // candidates are reconstructed at the centre of their quantisation step
    const unsigned xsub = (unsigned)(cx - 1) << 10;
    constexpr int KINF = 0x7f800000;
    auto thr_of = [&](float t) { const float tt = sqrtf(t) * 1.000001f + FEQ; return tt * tt * 1.000001f; };
    const float thr_r = thr_of((float)(r2 * g.inv_cell * g.inv_cell * (1024.0 * 1024.0)) * 1.000001f);
    int k1 = KINF, k2 = KINF, k3 = KINF, k4 = KINF;   // the four smallest keys, ascending
    int ord = 0;
    // four candidates per 16-byte gather; the distance arithmetic runs two candidates per instruction (v_pk_add / v_pk_mul /
    // v_pk_fma_f32: 6 packed instructions per pair instead of 12 scalar ones; lane-wise IEEE, so the keys are unchanged)
    typedef float v2f __attribute__((ext_vector_type(2)));
    // keys of four packed candidates for a query given by (qx_, xsub_, qyr, qzr), ordinals ord_ ..; the lanes of a wave also run this
    // for EACH OTHER's queries (pooled walk below): same expressions, same operand values, so the same keys whoever computes them
    auto keys4 = [&](const uint4_a4 W, int rem, float qx_, unsigned xsub_, float qyr, float qzr, int ord_, int (&keys)[4]) {
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const unsigned w0 = W[2 * h], w1 = W[2 * h + 1];
            v2f cx2 = {(float)((w0 - xsub_) & 4095u), (float)((w1 - xsub_) & 4095u)};
            v2f cy2 = {__uint_as_float((w0 & 0x003ff000u) | 0x45000000u), __uint_as_float((w1 & 0x003ff000u) | 0x45000000u)};
            v2f cz2 = {(float)(w0 >> 22), (float)(w1 >> 22)};
            const v2f qx2 = {qx_, qx_}, qy2 = {qyr + 2048.f, qyr + 2048.f}, qz2 = {qzr, qzr};
            const v2f fdx = cx2 - qx2, fdy = cy2 - qy2, fdz = cz2 - qz2;
            const v2f f = __builtin_elementwise_fma(fdz, fdz, __builtin_elementwise_fma(fdy, fdy, fdx * fdx));
            keys[2 * h] = (__float_as_int(f.x) & ~1023) | (ord_ + 2 * h);
            keys[2 * h + 1] = (__float_as_int(f.y) & ~1023) | (ord_ + 2 * h + 1);
        }
#pragma unroll
        for (int u = 0; u < 4; u++) keys[u] = u < rem ? keys[u] : KINF;
    };
    auto fold4 = [&](const int (&keys)[4]) {
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int key = keys[u];
            k4 = med3_i32(k3, k4, key);
            k3 = med3_i32(k2, k3, key);
            k2 = med3_i32(k1, k2, key);
            k1 = min(k1, key);
        }
    };
    auto scan4w = [&](const uint4_a4 W, int rem, float qyr, float qzr) {
        int keys[4];
        keys4(W, rem, qx, xsub, qyr, qzr, ord, keys);
        fold4(keys);
        ord += 4;
    };
    auto scan4 = [&](int j0, int e, float qyr, float qzr) { scan4w(*(const uint4_a4 *)(g.q10 + j0), e - j0, qyr, qzr); };
    // centre row first: it gives the pruning threshold for the other eight
    if (G == 1) {
        for (int j0 = rb[0]; j0 < re[0]; j0 += 4) scan4(j0, re[0], qyc - 1024.5f, qzc - 1024.5f);
    } else {
        for (int j0 = rb[0]; j0 < re[0]; j0 += 4 * G) {
            uint4_a4 W[G];
#pragma unroll
            for (int q = 0; q < G; q++) W[q] = *(const uint4_a4 *)(g.q10 + min(j0 + 4 * q, re[0] - 1));   // clamped: a group past the run is not used
#pragma unroll
            for (int q = 0; q < G; q++)
                if (j0 + 4 * q < re[0]) scan4w(W[q], re[0] - (j0 + 4 * q), qyc - 1024.5f, qzc - 1024.5f);
        }
    }
    const float thr = fminf(thr_r, thr_of(__int_as_float(k1 & ~1023)) * 1.0003f);   // (key truncation: the key is below f by < 2^-13)
    const bool trim = de == 3 && xa == x0;         // the run is exactly the cells cx-1, cx, cx+1 (no clamping at the grid border)
    const float sxl = (qxc - 1024.f) * (qxc - 1024.f), sxh = (2048.f - qxc) * (2048.f - qxc);
    // a record is two words: first slot, and length | row << 20 (lengths are below 1024); ordinal bases are the running sum of
    // the padded lengths, recomputed by the one decode at the end.  Record 0: the centre row (ordinal 0)
    sRun[tid] = rb[0];
    sRun[B + tid] = re[0] - rb[0];
    int nr = 1, myg = 0;                            // records, and groups of four candidates in the records after the centre row
#pragma unroll
    for (int q = 1; q < 9; q++) {
        const int r = ORD[q], ry = r % 3, rz = r / 3;
        const float sy = ry == 0 ? qyc - 1024.f : ry == 2 ? 2048.f - qyc : 0.f, sz = rz == 0 ? qzc - 1024.f : rz == 2 ? 2048.f - qzc : 0.f;
        const float syz = sy * sy + sz * sz;
        // a full run (cells cx-1, cx, cx+1) also drops an end cell that is too far in x
        const int b_ = trim && sxl + syz > thr ? rm1[q] : rb[q], e_ = trim && sxh + syz > thr ? rm2[q] : re[q];
        if (re[q] > rb[q] && e_ > b_ && syz <= thr) {   // (a row outside the grid has re == rb and meaningless cell boundaries)
            sRun[(nr * 2) * B + tid] = b_;
            sRun[(nr * 2 + 1) * B + tid] = (e_ - b_) | (r << 20);
            myg += (e_ - b_ + 3) >> 2;
            nr++;
        }
    }
    // POOLED WALK of the other rows (G == 1, large clouds).  Left to itself a wave walks its lists for as long as its longest lane:
    // 9.3 groups on average where its average lane has 2.3 (profiles/r04_icp_search_stats.log) -- three quarters of the wave's
    // lane-steps are idle.  Here the lanes put their groups into ONE queue of the wave (LDS), every lane computes the keys of every
    // (active-lane-count)-th group, whoever's query it belongs to -- the owner's query parameters travel through LDS, the
    // arithmetic is keys4() with the same operands, so the keys are the ones the owner would have computed -- and the owners
    // fold their groups' keys into their best four (4 instructions per candidate instead of 20).  A wave whose queue would
    // overflow (tot > POOL_Q: very dense cells) takes the per-lane walk below.
    bool pooled = false;
    if (G == 1 && sPool) {
        int *pw = sPool + (tid >> 6) * pool_words(POOL_Q);
        int *p_keys = pw, *p_item = pw + 4 * POOL_Q, *p_q = pw + 6 * POOL_Q, *p_tot = pw + 6 * POOL_Q + 256;
        const int lane = tid & 63;
        *(volatile int *)p_tot = 0;
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
        const int off = atomicAdd(p_tot, myg);                    // ds_add_rtn: a disjoint range of the queue per lane
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
        const int tot = *(volatile int *)p_tot;                   // the same for every lane of the wave
        if (tot <= POOL_Q) {
            pooled = true;
            p_q[lane] = __float_as_int(qx);
            p_q[64 + lane] = __float_as_int(qyc);
            p_q[128 + lane] = __float_as_int(qzc);
            p_q[192 + lane] = (int)xsub;
            int it = off, ob = ord;                               // ord: the centre row's padded length
            for (int k = 1; k < nr; k++) {
                const int jb = sRun[(k * 2) * B + tid], lr = sRun[(k * 2 + 1) * B + tid], len = lr & 0xfffff, r = lr >> 20;
                for (int o = 0; o < len; o += 4, it++) {
                    p_item[2 * it] = jb + o;
                    p_item[2 * it + 1] = lane | min(len - o, 4) << 6 | r << 9 | (ob + o) << 13;
                }
                ob += (len + 3) & ~3;
            }
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            __builtin_amdgcn_wave_barrier();
            const unsigned long long act = __ballot(1);
            const int nact = __popcll(act), rank = __popcll(act & ((1ull << lane) - 1ull));
            for (int i = rank; i < tot; i += nact) {
                const int j0 = p_item[2 * i], meta = p_item[2 * i + 1];
                const int o = meta & 63, rem = (meta >> 6) & 7, r = (meta >> 9) & 15, ordb = (int)((unsigned)meta >> 13);
                const float oqx = __int_as_float(p_q[o]), oqy = __int_as_float(p_q[64 + o]), oqz = __int_as_float(p_q[128 + o]);
                const unsigned oxs = (unsigned)p_q[192 + o];
                const int rz = (r * 11) >> 5, ry = r - 3 * rz;
                int keys[4];
                keys4(*(const uint4_a4 *)(g.q10 + j0), rem, oqx, oxs, oqy - 0.5f - 1024.f * (float)ry, oqz - 0.5f - 1024.f * (float)rz, ordb, keys);
                *(int4 *)(p_keys + 4 * i) = make_int4(keys[0], keys[1], keys[2], keys[3]);
            }
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            __builtin_amdgcn_wave_barrier();
            for (int gq = 0; gq < myg; gq++) {
                const int4 kk = *(const int4 *)(p_keys + 4 * (off + gq));
                const int keys[4] = {kk.x, kk.y, kk.z, kk.w};
                fold4(keys);
            }
        }
    }
    // PER-LANE WALK: every lane walks its own list.  With G == 1 this is the overflow fallback of the pooled walk (tot > POOL_Q),
    // with G == 3 it is the walk itself.
    if (!pooled) {
        int k = 1, j0 = 0, e = 0;
        float qyr = 0.f, qzr = 0.f;
        auto next_run = [&]() {     // false: the list is exhausted
            if (k >= nr) return false;
            j0 = sRun[(k * 2) * B + tid];
            const int lr = sRun[(k * 2 + 1) * B + tid];
            e = j0 + (lr & 0xfffff);
            const int r = lr >> 20;
            const int rz = (r * 11) >> 5, ry = r - 3 * rz;
            qyr = qyc - 0.5f - 1024.f * (float)ry;
            qzr = qzc - 0.5f - 1024.f * (float)rz;
            k++;
            return true;
        };
        if (G == 1) {
            for (;;) {
                if (j0 >= e && !next_run()) break;
                scan4(j0, e, qyr, qzr);
                j0 += 4;
            }
        } else {
            // walk the list G groups ahead (addresses and row constants only), request them all, then use them in the same order
            for (bool more = true; more;) {
                int aj[G], ar[G];
                float ay[G], az[G];
                int ng = 0;
#pragma unroll
                for (int q = 0; q < G; q++) {
                    aj[q] = 0; ar[q] = 0; ay[q] = 0.f; az[q] = 0.f;
                    if (more && j0 >= e) more = next_run();
                    if (more) { aj[q] = j0; ar[q] = e - j0; ay[q] = qyr; az[q] = qzr; j0 += 4; ng = q + 1; }
                }
                uint4_a4 W[G];
#pragma unroll
                for (int q = 0; q < G; q++) W[q] = *(const uint4_a4 *)(g.q10 + aj[q]);     // unused slots read entry 0
#pragma unroll
                for (int q = 0; q < G; q++)
                    if (q < ng) scan4w(W[q], ar[q], ay[q], az[q]);
            }
        }
    }
    if (k1 == KINF) return;                        // nothing scanned: the caller goes on to the outer shells
    const float t1 = __int_as_float(k1 | 1023);    // upper end of the key's truncation interval
    const float thr2 = thr_of(t1) * 1.0003f;
    if (__int_as_float(k4 & ~1023) <= thr2) {      // a fourth contender: the triple may be incomplete
        nn_block_global(g, px, py, pz, cx, cy, cz, best, bi);
        return;
    }
    // ordinal -> slot: the record with the largest ordinal base not above it.  The best candidate is always evaluated; the
    // second and third only when they lie inside the margin (about one query in a hundred), in a branch of their own
    auto slot_of = [&](int o) {
        int jb = sRun[tid], ob = 0, next = ((sRun[B + tid] & 0xfffff) + 3) & ~3;
        for (int k = 1; k < nr; k++) {
            const int b_ = sRun[(k * 2) * B + tid], o_ = next;
            next += ((sRun[(k * 2 + 1) * B + tid] & 0xfffff) + 3) & ~3;
            if (o >= o_) { jb = b_; ob = o_; }
        }
        return jb + (o - ob);
    };
    auto exact = [&](int j) {
        const double dx = g.pts[(int64_t)j * 3] - px, dy = g.pts[(int64_t)j * 3 + 1] - py, dz = g.pts[(int64_t)j * 3 + 2] - pz;
        const double d2 = dx * dx + dy * dy + dz * dz;
        if (d2 <= best) {
            if (d2 < best || (bi >= 0 && g.idx[j] < g.idx[bi])) { best = d2; bi = j; }
        }
    };
    exact(slot_of(k1 & 1023));
    if (k2 != KINF && __int_as_float(k2 & ~1023) <= thr2) {
        exact(slot_of(k2 & 1023));
        if (k3 != KINF && __int_as_float(k3 & ~1023) <= thr2) exact(slot_of(k3 & 1023));
    }
}

// shells 2.. of the 1-NN search (only queries whose nearest point is further than one cell away get here: most of them in the
// first evaluation of an unaligned pair, a handful per million afterwards), by pruned x-rows (for_shell_rows); the result does
// not depend on the visiting order because of the total order (d2, index).
__device__ __forceinline__ void nn_outer_shells(const GridView &g, double px, double py, double pz, int cx, int cy, int cz, int smax,
                                                double &best, int &bi) {
    auto visit = [&](int b, int e) {
        for (int j0 = b; j0 < e; j0 += 4) {       // four candidates per round trip, clamped slots (no branch around a load)
            double X[4], Y[4], Z[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int64_t jj = min(j0 + u, e - 1);
                X[u] = g.pts[jj * 3]; Y[u] = g.pts[jj * 3 + 1]; Z[u] = g.pts[jj * 3 + 2];
            }
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int j = j0 + u;
                const double dx = X[u] - px, dy = Y[u] - py, dz = Z[u] - pz;
                const double d2 = dx * dx + dy * dy + dz * dz;
                if (j < e && d2 <= best) {
                    if (d2 < best || (bi >= 0 && g.idx[j] < g.idx[bi])) { best = d2; bi = j; }
                }
            }
        }
    };
    for (int s = 1; s <= max(smax, 1); s++) {
        if (s > 1) for_shell_rows(g, px, py, pz, cx, cy, cz, s, [&]() { return best; }, visit);
        const double reach = s * g.cell;
        if (bi >= 0 && best <= reach * reach) break;
    }
}

// adds one correspondence (source point i at p, target slot bi at squared distance `best`) to the accumulators
template <int MODE>
__device__ __forceinline__ void icp_accumulate(const GridView &g, const double *__restrict__ src_n, const double *__restrict__ tgt_n,
                                               int64_t i, const Rigid &T, double eps, double px, double py, double pz, double best, int bi,
                                               double (&acc)[29], const IcpColor &col, const IcpOrigin &o) {
        const double tx = g.pts[(int64_t)bi * 3], ty = g.pts[(int64_t)bi * 3 + 1], tz = g.pts[(int64_t)bi * 3 + 2];
        acc[0] += 1.0;
        acc[1] += best;
        if (MODE == MODE_P2P) {
            // moments relative to the centre of the target grid's box (a correspondence is within max_dist of that box):
            // sigma = E[p t^T] - mean mean^T cancels against the clouds' extent, not against their distance from the world
            // origin.  k_icp_step restores the translation.
            const double qx = px - o.x, qy = py - o.y, qz = pz - o.z;
            const double ux = tx - o.x, uy = ty - o.y, uz = tz - o.z;
            acc[2] += qx; acc[3] += qy; acc[4] += qz;
            acc[5] += ux; acc[6] += uy; acc[7] += uz;
            acc[8] += qx * ux; acc[9] += qx * uy; acc[10] += qx * uz;
            acc[11] += qy * ux; acc[12] += qy * uy; acc[13] += qy * uz;
            acc[14] += qz * ux; acc[15] += qz * uy; acc[16] += qz * uz;
        } else {
            double J[3][6], rr[3];
            int rows;
            const double nx = tgt_n[(int64_t)bi * 3], ny = tgt_n[(int64_t)bi * 3 + 1], nz = tgt_n[(int64_t)bi * 3 + 2];
            const double dx = px - tx, dy = py - ty, dz = pz - tz;
            if (MODE == MODE_P2PLANE) {
                rows = 1;
                J[0][0] = py * nz - pz * ny; J[0][1] = pz * nx - px * nz; J[0][2] = px * ny - py * nx;
                J[0][3] = nx; J[0][4] = ny; J[0][5] = nz;
                rr[0] = dx * nx + dy * ny + dz * nz;
#pragma unroll
                for (int a = 0, q = 2; a < 6; a++)
#pragma unroll
                    for (int b = a; b < 6; b++, q++) acc[q] += J[0][a] * J[0][b];
#pragma unroll
                for (int a = 0; a < 6; a++) acc[23 + a] += J[0][a] * rr[0];
            } else if (MODE == MODE_COLORED) {
                rows = 2;
                (void)rows;
                const double e = dx * nx + dy * ny + dz * nz;
                // geometric row: point-to-plane's, scaled (sg = 1 leaves every product as point-to-plane forms it)
                J[0][0] = col.sg * (py * nz - pz * ny); J[0][1] = col.sg * (pz * nx - px * nz); J[0][2] = col.sg * (px * ny - py * nx);
                J[0][3] = col.sg * nx; J[0][4] = col.sg * ny; J[0][5] = col.sg * nz;
                rr[0] = col.sg * e;
                // photometric row
                const double *ig = col.tgt_ig + (int64_t)bi * 4;
                const double it = ig[0], gx = ig[1], gy = ig[2], gz = ig[3];
                const double is = col.src_i[i];
                const double gn = gx * nx + gy * ny + gz * nz;
                const double mx = -(gx - gn * nx), my = -(gy - gn * ny), mz = -(gz - gn * nz);
                const double i0 = (gx * ((px - e * nx) - tx) + gy * ((py - e * ny) - ty) + gz * ((pz - e * nz) - tz)) + it;
                J[1][0] = col.sp * (py * mz - pz * my); J[1][1] = col.sp * (pz * mx - px * mz); J[1][2] = col.sp * (px * my - py * mx);
                J[1][3] = col.sp * mx; J[1][4] = col.sp * my; J[1][5] = col.sp * mz;
                rr[1] = col.sp * (is - i0);
#pragma unroll
                for (int a = 0, q = 2; a < 6; a++)
#pragma unroll
                    for (int b = a; b < 6; b++, q++) { acc[q] += J[0][a] * J[0][b]; acc[q] += J[1][a] * J[1][b]; }
#pragma unroll
                for (int a = 0; a < 6; a++) { acc[23 + a] += J[0][a] * rr[0]; acc[23 + a] += J[1][a] * rr[1]; }
            } else {
                rows = 3;
                (void)rows;
                // effective normals (QUIRK of GetRotationFromE1ToX: n.e1 < -0.99 -> e1)
                double ax = nx, ay = ny, az = nz;
                if (ax < -0.99) { ax = 1; ay = 0; az = 0; }
                double ux = src_n[i * 3], uy = src_n[i * 3 + 1], uz = src_n[i * 3 + 2];
                if (ux < -0.99) { ux = 1; uy = 0; uz = 0; }
                const double bx = T.r[0] * ux + T.r[1] * uy + T.r[2] * uz, by = T.r[3] * ux + T.r[4] * uy + T.r[5] * uz,
                             bz = T.r[6] * ux + T.r[7] * uy + T.r[8] * uz;
                const double w = 1.0 - eps;
                double M[6] = {2.0 - w * (ax * ax + bx * bx), -w * (ax * ay + bx * by), -w * (ax * az + bx * bz),
                               2.0 - w * (ay * ay + by * by), -w * (ay * az + by * bz), 2.0 - w * (az * az + bz * bz)};
                double A[6];
                if (!inv3_sym(M, A)) return;
                // Jb = [K | I], K = -[p]x ; G = A * Jb (3x6) ; JtJ = Jb^T G ; Jtr = Jb^T (A d).
                // Written out by blocks: K has one zero per row and column and the right half of Jb is the identity; spelled as
                // dense 3-term products those zeros and ones are real float64 multiplies (0 * x is not foldable under IEEE rules),
                // a third of this function's arithmetic.  Dropping an exact-zero term of a sum leaves the sum unchanged bit for bit:
                //   K = [0 pz -py; -pz 0 px; py -px 0],  AK[a][b] = sum_c A[a][c] K[c][b],  JtJ = [K^T A K, K^T A; A K, A]
                const double As[3][3] = {{A[0], A[1], A[2]}, {A[1], A[3], A[4]}, {A[2], A[4], A[5]}};
                double AK[3][3];
#pragma unroll
                for (int a = 0; a < 3; a++) {
                    AK[a][0] = As[a][1] * -pz + As[a][2] * py;
                    AK[a][1] = As[a][0] * pz + As[a][2] * -px;
                    AK[a][2] = As[a][0] * -py + As[a][1] * px;
                }
                const double Ad[3] = {As[0][0] * dx + As[0][1] * dy + As[0][2] * dz, As[1][0] * dx + As[1][1] * dy + As[1][2] * dz,
                                      As[2][0] * dx + As[2][1] * dy + As[2][2] * dz};
                // rows of K^T X for a 3-vector of rows X[0..2]: (K^T X)[0] = -pz X[1] + py X[2], [1] = pz X[0] - px X[2], [2] = -py X[0] + px X[1]
                // slots: q = 2 + index of (a, b), a <= b, row-major over the upper triangle of the 6x6
                // a = 0: b = 0..5
                acc[2] += -pz * AK[1][0] + py * AK[2][0];
                acc[3] += -pz * AK[1][1] + py * AK[2][1];
                acc[4] += -pz * AK[1][2] + py * AK[2][2];
                acc[5] += -pz * As[1][0] + py * As[2][0];
                acc[6] += -pz * As[1][1] + py * As[2][1];
                acc[7] += -pz * As[1][2] + py * As[2][2];
                // a = 1: b = 1..5
                acc[8] += pz * AK[0][1] + -px * AK[2][1];
                acc[9] += pz * AK[0][2] + -px * AK[2][2];
                acc[10] += pz * As[0][0] + -px * As[2][0];
                acc[11] += pz * As[0][1] + -px * As[2][1];
                acc[12] += pz * As[0][2] + -px * As[2][2];
                // a = 2: b = 2..5
                acc[13] += -py * AK[0][2] + px * AK[1][2];
                acc[14] += -py * As[0][0] + px * As[1][0];
                acc[15] += -py * As[0][1] + px * As[1][1];
                acc[16] += -py * As[0][2] + px * As[1][2];
                // a = 3..5: the rows of A itself
                acc[17] += As[0][0]; acc[18] += As[0][1]; acc[19] += As[0][2];
                acc[20] += As[1][1]; acc[21] += As[1][2];
                acc[22] += As[2][2];
                acc[23] += -pz * Ad[1] + py * Ad[2];
                acc[24] += pz * Ad[0] + -px * Ad[2];
                acc[25] += -py * Ad[0] + px * Ad[1];
                acc[26] += Ad[0]; acc[27] += Ad[1]; acc[28] += Ad[2];
            }
        }
    
}

// the three forms of the correspondence search (the values are part of the kernels' symbol names)
enum { SEARCH_EXACT = 0 /* nn_block_global */, SEARCH_Q10 = 2 /* nn_block_q10<1>, pooled walk */, SEARCH_Q10_DEEP = 3 /* nn_block_q10<3>: small clouds */ };
template <int MODE, int SEARCH>
__global__ void __launch_bounds__(ICP_BLOCK, SEARCH == SEARCH_Q10_DEEP ? 2 : 3) k_icp_eval(GridView g, const double *__restrict__ src, const double *__restrict__ src_n,
                                                        const double *__restrict__ tgt_n /* cell-sorted order */, int64_t ns,
                                                        const IcpState *__restrict__ st, double max_dist, double eps, double *__restrict__ partial,
                                                        int *__restrict__ corr /* optional [ns] target original index or -1 */,
                                                        IcpColor col /* MODE_COLORED only */, IcpOrigin org /* MODE_P2P only */) {
    static_assert(ICP_BLOCK == 256, "nn_block_q10 assumes 256 threads");
    __shared__ int sRun[SEARCH >= SEARCH_Q10 ? 18 * ICP_BLOCK : 1];
    __shared__ __attribute__((aligned(16))) int sPoolBuf[SEARCH == SEARCH_Q10 ? (ICP_BLOCK / 64) * pool_words(POOL_Q) : 4];
    int *const sPool = SEARCH == SEARCH_Q10 && g.pool ? sPoolBuf : nullptr;
    if (st->done) return;                        // the loop ended in an earlier launch of this batch (uniform)
    const Rigid T = load_rigid(st);
    double acc[ICP_SLOTS];
#pragma unroll
    for (int q = 0; q < ICP_SLOTS; q++) acc[q] = 0;
    const double r2 = max_dist * max_dist;
    const int smax = (int)ceil(max_dist * g.inv_cell);
    // XCD-aware share of the queries: workgroups go round-robin to the eight XCDs, each with an L2 of its own; the source is in
    // Morton order of the target cells, so giving XCD x the x-th eighth of the chunks (256 consecutive queries) confines the
    // target data an L2 sees (cell table, packed candidates, points, normals) to an eighth of the cloud
    const int64_t nchunk = (ns + ICP_BLOCK - 1) / ICP_BLOCK;
    int64_t c_begin = blockIdx.x, c_end = nchunk, c_step = gridDim.x;
    if ((gridDim.x & 7) == 0) {
        const int x = blockIdx.x & 7;
        c_begin = x * nchunk / 8 + (blockIdx.x >> 3);
        c_end = (x + 1) * nchunk / 8;
        c_step = gridDim.x >> 3;
    }
    for (int64_t c = c_begin; c < c_end; c += c_step) {
        const int64_t i = c * ICP_BLOCK + threadIdx.x;
        if (i >= ns) continue;
        double px, py, pz;
        rigid_apply(T, src[i * 3], src[i * 3 + 1], src[i * 3 + 2], px, py, pz);
        const int cx = cell_coord(px, g.ox, g.inv_cell), cy = cell_coord(py, g.oy, g.inv_cell), cz = cell_coord(pz, g.oz, g.inv_cell);
        double best = r2;
        int bi = -1;
        if (SEARCH == SEARCH_Q10_DEEP) nn_block_q10<3>(g, px, py, pz, cx, cy, cz, r2, best, bi, sRun);
        else if (SEARCH == SEARCH_Q10) nn_block_q10<1>(g, px, py, pz, cx, cy, cz, r2, best, bi, sRun, sPool);
        else nn_block_global(g, px, py, pz, cx, cy, cz, best, bi);
        nn_outer_shells(g, px, py, pz, cx, cy, cz, smax, best, bi);
        if (corr) corr[i] = bi >= 0 ? g.idx[bi] : -1;
        if (bi >= 0) icp_accumulate<MODE>(g, src_n, tgt_n, i, T, eps, px, py, pz, best, bi, acc, col, org);
    }
    __shared__ double sm[ICP_BLOCK / 64][ICP_SLOTS];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < ICP_SLOTS; q++) {
        double v = wave_sum(acc[q]);
        if (lane == 0) sm[wv][q] = v;
    }
    __syncthreads();
    if (threadIdx.x < ICP_SLOTS) {
        double v = 0;
        for (int w2 = 0; w2 < ICP_BLOCK / 64; w2++) v += sm[w2][threadIdx.x];
        partial[(size_t)threadIdx.x * gridDim.x + blockIdx.x] = v;   // [slot][workgroup]: the step kernel reads a slot's sums as one contiguous run
    }
}

// r3d_debug_icp_correspondences: brings one evaluation's correspondences back to the caller's numbering.  `corr` is indexed by the
// Morton-sorted source and holds target original indices (k_icp_eval's corr); `perm` is the source sort.  The squared distance
// is recomputed with the search's own expression.
__global__ void __launch_bounds__(256) k_icp_corr_readout(const double *__restrict__ src, const int *__restrict__ perm, int64_t ns,
                                                          const IcpState *__restrict__ st, const double *__restrict__ tgt /* caller's order */,
                                                          const int *__restrict__ corr, int *__restrict__ corr_out, double *__restrict__ d2_out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= ns) return;
    const Rigid T = load_rigid(st);
    const int c = corr[i];
    double d2 = 1e300;
    if (c >= 0) {
        double px, py, pz;
        rigid_apply(T, src[i * 3], src[i * 3 + 1], src[i * 3 + 2], px, py, pz);
        const double dx = tgt[(int64_t)c * 3] - px, dy = tgt[(int64_t)c * 3 + 1] - py, dz = tgt[(int64_t)c * 3 + 2] - pz;
        d2 = dx * dx + dy * dy + dz * dz;
    }
    const int o = perm[i];
    corr_out[o] = c;
    d2_out[o] = d2;
}

__global__ void __launch_bounds__(256) k_transform(const double *__restrict__ in, int64_t n, Rigid T, int rotate_only, double *__restrict__ out) {
    int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double x = in[i * 3], y = in[i * 3 + 1], z = in[i * 3 + 2];
    const double tx = rotate_only ? 0 : T.t[0], ty = rotate_only ? 0 : T.t[1], tz = rotate_only ? 0 : T.t[2];
    out[i * 3] = T.r[0] * x + T.r[1] * y + T.r[2] * z + tx;
    out[i * 3 + 1] = T.r[3] * x + T.r[4] * y + T.r[5] * z + ty;
    out[i * 3 + 2] = T.r[6] * x + T.r[7] * y + T.r[8] * z + tz;
}

// k_transform over a count that is still on the device (see k_bbox_partial_dn); the grid covers the upper bound
__global__ void __launch_bounds__(256) k_transform_dn(const double *__restrict__ in, const int *__restrict__ c0, const int *__restrict__ c1, Rigid T,
                                                      double *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)*c0 + *c1) return;
    rigid_apply(T, in[i * 3], in[i * 3 + 1], in[i * 3 + 2], out[i * 3], out[i * 3 + 1], out[i * 3 + 2]);
}

// several blocks of triplets, each with its own rigid transform, in ONE launch (the fuse step of the multi-view exchange: eight
// views x (points, normals) were sixteen launches of ~2 us of work each behind ~18 us of host call overhead each)
constexpr int TB_MAX = 16;
struct TransformBlocks {
    const double *in[TB_MAX];
    double *out[TB_MAX];
    long long end[TB_MAX];      // running end offset of block b in the concatenated index space
    double r[TB_MAX][12];       // row-major 3x3 + translation (zero for rotate-only blocks)
    int n;
};
__global__ void __launch_bounds__(256) k_transform_blocks(TransformBlocks B) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= B.end[B.n - 1]) return;
    int b = 0;
#pragma unroll
    for (int q = 0; q < TB_MAX - 1; q++) b += (q < B.n - 1 && i >= B.end[q]) ? 1 : 0;
    const long long j = i - (b ? B.end[b - 1] : 0);
    const double *in = B.in[b];
    double *out = B.out[b];
    const double *r = B.r[b];
    const double x = in[j * 3], y = in[j * 3 + 1], z = in[j * 3 + 2];
    out[j * 3] = r[0] * x + r[1] * y + r[2] * z + r[9];          // the evaluation order of k_transform
    out[j * 3 + 1] = r[3] * x + r[4] * y + r[5] * z + r[10];
    out[j * 3 + 2] = r[6] * x + r[7] * y + r[8] * z + r[11];
}

// ------------------------------------------------------------------------------------------------ disparity -> cloud
// cv2.reprojectImageTo3D semantics: [X Y Z W]^T = Q [x y d 1]^T, point = (X, Y, Z) / W with d = disp / 16;
// pixels with disp < min_valid (the matcher's invalid marker and anything below minDisparity) are dropped.
__global__ void __launch_bounds__(256) k_disp_flags(const int16_t *__restrict__ disp, int64_t n, int min_valid, int *__restrict__ flags) {
    int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) flags[i] = disp[i] >= min_valid ? 1 : 0;
}
struct Mat4 { double m[16]; };
// same, and additionally |Z/W| <= max_depth (the value k_reproject will write, computed by the same expressions)
__global__ void __launch_bounds__(256) k_disp_flags_depth(const int16_t *__restrict__ disp, int w, int64_t n, int min_valid, Mat4 Q,
                                                         double max_depth, int *__restrict__ flags) {
    int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double x = (double)(i % w), y = (double)(i / w), d = (double)disp[i] / 16.0;
    const double Z = Q.m[8] * x + Q.m[9] * y + Q.m[10] * d + Q.m[11];
    const double W = Q.m[12] * x + Q.m[13] * y + Q.m[14] * d + Q.m[15];
    flags[i] = (disp[i] >= min_valid && fabs(Z / W) <= max_depth) ? 1 : 0;
}
__global__ void __launch_bounds__(256) k_reproject(const int16_t *__restrict__ disp, const int *__restrict__ flags, const int *__restrict__ scan,
                                                   int w, int64_t n, Mat4 Q, double *__restrict__ xyz, int *__restrict__ pix) {
    int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n || !flags[i]) return;
    const double x = (double)(i % w), y = (double)(i / w), d = (double)disp[i] / 16.0;
    const double X = Q.m[0] * x + Q.m[1] * y + Q.m[2] * d + Q.m[3];
    const double Y = Q.m[4] * x + Q.m[5] * y + Q.m[6] * d + Q.m[7];
    const double Z = Q.m[8] * x + Q.m[9] * y + Q.m[10] * d + Q.m[11];
    const double W = Q.m[12] * x + Q.m[13] * y + Q.m[14] * d + Q.m[15];
    const int64_t o = scan[i];
    xyz[o * 3] = X / W; xyz[o * 3 + 1] = Y / W; xyz[o * 3 + 2] = Z / W;
    if (pix) pix[o] = (int)i;
}
// colours of the compacted points (no voxel grid): one thread per point
template <int CN>
__global__ void __launch_bounds__(256) k_gather_colors(MemberColor<CN> ld, int64_t m, double *__restrict__ rgb) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    double r, g, b;
    ld.value(ld.fetch(i), r, g, b);
    rgb[i * 3] = r; rgb[i * 3 + 1] = g; rgb[i * 3 + 2] = b;
}

// ------------------------------------------------------------------------------------------------ depth image -> cloud
// open3d.geometry.PointCloud.create_from_rgbd_image(RGBDImage.create_from_color_and_depth(color, depth, depth_scale, depth_trunc,
// convert_rgb_to_intensity=False), intrinsic) followed by the flip of test/check84.py:155-159,172-178 -- the rule SURVEY.md
// Appendix C verified on all 163 recorded frames: z = float(raw) / float(depth_scale) in FLOAT32, (double)z >= depth_trunc
// ([recalled] Image::ConvertDepthToFloatImage clips `*p >= depth_trunc`, the float promoted to the double parameter; the recorded
// frames cannot tell >= from > because their scale 1/float(0.001) puts raw 3000 at 3.0000002) or z == 0 dropped, x = (u - ppx) z / fx, y = (v - ppy) z / fy in float64 (u = column, v = row), then (x, -y, -z); row-major pixel order;
// colours = channel / 255.
struct DepthCam { double fx, fy, ppx, ppy, trunc; float scale; int flip; };
__device__ __forceinline__ float depth_z(unsigned short raw, const DepthCam &c) {
    const float z = (float)raw / c.scale;
    return (double)z >= c.trunc ? 0.0f : z;
}
__global__ void __launch_bounds__(256) k_depth_flags(const unsigned short *__restrict__ depth, int w, int stride, int64_t n, DepthCam c,
                                                     int *__restrict__ flags) {
    int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    flags[i] = depth_z(depth[(i / w) * stride + (i % w)], c) > 0.0f ? 1 : 0;
}
__global__ void __launch_bounds__(256) k_backproject(const unsigned short *__restrict__ depth, const unsigned char *__restrict__ color,
                                                     const int *__restrict__ flags, const int *__restrict__ scan, int w, int stride,
                                                     int cstride, int64_t n, DepthCam c, double *__restrict__ xyz, double *__restrict__ rgb,
                                                     int *__restrict__ pix) {
    int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n || !flags[i]) return;
    const int u = (int)(i % w), v = (int)(i / w);
    const double z = (double)depth_z(depth[(int64_t)v * stride + u], c);
    const double x = ((double)u - c.ppx) * z / c.fx, y = ((double)v - c.ppy) * z / c.fy;
    const int64_t o = scan[i];
    xyz[o * 3] = x; xyz[o * 3 + 1] = c.flip ? -y : y; xyz[o * 3 + 2] = c.flip ? -z : z;
    if (rgb) {
        const unsigned char *p = color + (int64_t)v * cstride + 3 * u;
        rgb[o * 3] = (double)p[0] / 255.0; rgb[o * 3 + 1] = (double)p[1] / 255.0; rgb[o * 3 + 2] = (double)p[2] / 255.0;
    }
    if (pix) pix[o] = (int)i;
}

// ------------------------------------------------------------------------------------------------ incremental model voxel table
// The scanning loop re-down-samples the WHOLE model every frame (pointcloud_alignment.py:23; main.py:48).  The legacy grid's voxel
// of a point depends only on the model's minimum corner (origin = min_bound - voxel / 2) and a voxel's mean is its members summed
// in index order, so while the minimum corner stays put, a frame appended at the END of the model only continues running sums:
// the table keeps, per occupied voxel in lexicographic (kx, ky, kz) order, the packed key, the running float64 sums and the
// count; a new frame's points are sorted by (voxel, index), every run is added member by member onto its voxel's running sum
// (or starts a new voxel from zero), and the new voxels are merged into the sorted table.  means = sums / count are then bit for
// bit those of a full re-voxelisation (tests/test_pipeline_gpu.py asserts it on a recorded scan, tests/test_voxel_edges_gpu.py
// entry by entry through r3d_model_debug_voxel_table; R3D_MODEL_IMPL=rebuild keeps the full pass).
__device__ __forceinline__ unsigned long long vt_key_of(const double *__restrict__ p, double ox, double oy, double oz, double voxel) {
    const long long kx = (long long)floor((p[0] - ox) / voxel), ky = (long long)floor((p[1] - oy) / voxel), kz = (long long)floor((p[2] - oz) / voxel);
    return (unsigned long long)kx << 42 | (unsigned long long)ky << 21 | (unsigned long long)kz;   // each index < 2^21 (checked on the host)
}
// table from scratch: one thread per voxel segment of the (voxel, index)-sorted model (the loop of k_voxel_mean_sorted)
template <int R>
__global__ void __launch_bounds__(256) k_vt_build(const double *__restrict__ sp, const int *__restrict__ starts, int64_t nseg, int64_t n, double ox,
                                                  double oy, double oz, double voxel, unsigned long long *__restrict__ keys,
                                                  double *__restrict__ sums, int *__restrict__ cnt) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= nseg) return;
    const int b = starts[s], e = s + 1 < nseg ? starts[s + 1] : (int)n, m = e - b;
    const double *__restrict__ p = sp + (int64_t)b * 3;
    double x = 0, y = 0, z = 0;
    double cur[3 * R], nxt[3 * R];
#pragma unroll
    for (int u = 0; u < R; u++) {
        const int64_t q = (int64_t)min(u, m - 1) * 3;
        cur[u * 3] = p[q]; cur[u * 3 + 1] = p[q + 1]; cur[u * 3 + 2] = p[q + 2];
    }
    keys[s] = vt_key_of(cur, ox, oy, oz, voxel);
    for (int i0 = 0; i0 < m; i0 += R) {
#pragma unroll
        for (int u = 0; u < R; u++) {
            const int64_t q = (int64_t)min(i0 + R + u, m - 1) * 3;
            nxt[u * 3] = p[q]; nxt[u * 3 + 1] = p[q + 1]; nxt[u * 3 + 2] = p[q + 2];
        }
#pragma unroll
        for (int u = 0; u < R; u++)
            if (i0 + u < m) { x += cur[u * 3]; y += cur[u * 3 + 1]; z += cur[u * 3 + 2]; }
#pragma unroll
        for (int u = 0; u < 3 * R; u++) cur[u] = nxt[u];
    }
    sums[s * 3] = x; sums[s * 3 + 1] = y; sums[s * 3 + 2] = z;
    cnt[s] = m;
}
__device__ __forceinline__ int64_t vt_lower_bound(const unsigned long long *__restrict__ keys, int64_t n, unsigned long long k) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (keys[mid] < k) lo = mid + 1; else hi = mid;
    }
    return lo;
}
// one thread per run of the sorted slice: continue the voxel's running sum in place, or start a new voxel
__global__ void __launch_bounds__(256) k_vt_update(const double *__restrict__ sp, const int *__restrict__ starts, int64_t nseg, int64_t n, double ox,
                                                   double oy, double oz, double voxel, const unsigned long long *__restrict__ tkeys, int64_t tn,
                                                   double *__restrict__ tsums, int *__restrict__ tcnt, unsigned long long *__restrict__ segkey,
                                                   int *__restrict__ is_new, int64_t *__restrict__ ins, double *__restrict__ nsum, int *__restrict__ ncnt) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= nseg) return;
    const int b = starts[s], e = s + 1 < nseg ? starts[s + 1] : (int)n;
    const double *__restrict__ p = sp + (int64_t)b * 3;
    const unsigned long long k = vt_key_of(p, ox, oy, oz, voxel);
    const int64_t pos = vt_lower_bound(tkeys, tn, k);
    const bool found = pos < tn && tkeys[pos] == k;
    double x = 0, y = 0, z = 0;
    if (found) { x = tsums[pos * 3]; y = tsums[pos * 3 + 1]; z = tsums[pos * 3 + 2]; }
    for (int i = 0; i < e - b; i++) { x += p[(int64_t)i * 3]; y += p[(int64_t)i * 3 + 1]; z += p[(int64_t)i * 3 + 2]; }
    segkey[s] = k;
    is_new[s] = found ? 0 : 1;
    ins[s] = pos;
    if (found) {
        tsums[pos * 3] = x; tsums[pos * 3 + 1] = y; tsums[pos * 3 + 2] = z;
        tcnt[pos] += e - b;
    } else {
        nsum[s * 3] = x; nsum[s * 3 + 1] = y; nsum[s * 3 + 2] = z;
        ncnt[s] = e - b;
    }
}
// merge: old voxel i moves up by the number of NEW keys below it; new voxel s goes to (old keys below it) + (new keys below it)
__global__ void __launch_bounds__(256) k_vt_merge(const unsigned long long *__restrict__ tkeys, const double *__restrict__ tsums, const int *__restrict__ tcnt,
                                                  int64_t tn, const unsigned long long *__restrict__ segkey, const int *__restrict__ is_new,
                                                  const int *__restrict__ rank /* exclusive scan of is_new */, const int64_t *__restrict__ ins,
                                                  const double *__restrict__ nsum, const int *__restrict__ ncnt, int64_t nseg, int total_new,
                                                  unsigned long long *__restrict__ okeys, double *__restrict__ osums, int *__restrict__ ocnt) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < tn) {
        const unsigned long long k = tkeys[i];
        const int64_t lb = vt_lower_bound(segkey, nseg, k);          // runs with a smaller key
        const int64_t pos = i + (lb < nseg ? rank[lb] : total_new);
        okeys[pos] = k;
        osums[pos * 3] = tsums[i * 3]; osums[pos * 3 + 1] = tsums[i * 3 + 1]; osums[pos * 3 + 2] = tsums[i * 3 + 2];
        ocnt[pos] = tcnt[i];
    } else if (i < tn + nseg) {
        const int64_t s = i - tn;
        if (!is_new[s]) return;
        const int64_t pos = ins[s] + rank[s];
        okeys[pos] = segkey[s];
        osums[pos * 3] = nsum[s * 3]; osums[pos * 3 + 1] = nsum[s * 3 + 1]; osums[pos * 3 + 2] = nsum[s * 3 + 2];
        ocnt[pos] = ncnt[s];
    }
}
__global__ void __launch_bounds__(256) k_vt_means(const double *__restrict__ sums, const int *__restrict__ cnt, int64_t n, double *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double c = (double)cnt[i];
    out[i * 3] = sums[i * 3] / c; out[i * 3 + 1] = sums[i * 3 + 1] / c; out[i * 3 + 2] = sums[i * 3 + 2] / c;
}

// Small device -> host reads between kernels (counts, bounding boxes).  k_publish copies every piece into the context's pinned,
// device-mapped buffer and then stores a sequence number there (system-scope fence in between); the host polls that number in
// memory.  No copy command, no marker, no runtime call in the wait: two staged 4-byte hipMemcpyAsync + a blocking synchronise
// cost ~50 us of idle GPU per round trip, two pinned copies + an event poll ~25 us (and were, in the registration loop, the part
// whose completion sometimes reached the host tens of milliseconds late), this form ~15 us.
struct PubDesc { const void *src[8]; unsigned off[8], bytes[8]; int n; unsigned seq; };
__global__ void __launch_bounds__(256) k_publish(PubDesc d, char *__restrict__ host) {
    for (int q = 0; q < d.n; q++) {
        const char *s = (const char *)d.src[q];
        for (unsigned i = threadIdx.x * 4; i < d.bytes[q]; i += 256 * 4) *(int *)(host + d.off[q] + i) = *(const int *)(s + i);
    }
    // every writer makes its stores visible at system scope, the barrier orders them before thread 0, which releases once more before
    // the sequence number goes out (PCIe keeps posted writes of one device in order)
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0) {
        __threadfence_system();
        *(volatile unsigned *)host = d.seq;
    }
}
struct PinRead {
    r3d_ctx *ctx;
    size_t off = 64;   // the first 64 bytes of the buffer hold the sequence number
    PubDesc d;
    void *host[8];
    explicit PinRead(r3d_ctx *c) : ctx(c) { d.n = 0; }
    int add(void *host_dst, const void *dev, size_t bytes) {   // bytes: a multiple of 4
        if (!ctx->pin.p) {
            hipError_t e = ctx->pin.alloc(R3D_PIN_BYTES, hipHostMallocMapped);
            if (e != hipSuccess) return r3d_fail(ctx, R3D_E_OOM, "hipHostMalloc(%d) failed: %s", R3D_PIN_BYTES, hipGetErrorString(e));
            memset(ctx->pin.p, 0, 64);
        }
        if (d.n >= 8 || (bytes & 3) || off + bytes > R3D_PIN_BYTES) return r3d_fail(ctx, R3D_E_HIP, "PinRead: too much for one read-back");
        d.src[d.n] = dev; d.off[d.n] = (unsigned)off; d.bytes[d.n] = (unsigned)bytes;
        host[d.n++] = host_dst;
        off += (bytes + 15) & ~(size_t)15;
        return R3D_OK;
    }
    int wait() {
        char *dpin = nullptr;
        R3D_HIP(ctx, hipHostGetDevicePointer((void **)&dpin, ctx->pin.p, 0));
        d.seq = ++ctx->pin_seq;
        k_publish<<<1, 256, 0, ctx->stream>>>(d, dpin);
        R3D_HIP(ctx, hipGetLastError());
        // the read is a few microseconds away: poll the sequence number briefly, then wait properly (a blocking synchronise may put
        // the thread to sleep for a scheduler tick)
        const auto t0 = std::chrono::steady_clock::now();
        bool done = false;
        for (unsigned spins = 0; !done; spins++) {
            if (*(volatile unsigned *)ctx->pin.p == d.seq) { done = true; break; }
            if ((spins & 255) == 255 && std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > 1e-3) break;
        }
        if (!done) {
            R3D_HIP(ctx, hipStreamSynchronize(ctx->stream));
            if (*(volatile unsigned *)ctx->pin.p != d.seq) return r3d_fail(ctx, R3D_E_HIP, "PinRead: the published sequence number did not arrive");
        }
        std::atomic_thread_fence(std::memory_order_acquire);
        for (int i = 0; i < d.n; i++) memcpy(host[i], (const char *)ctx->pin.p + d.off[i], d.bytes[i]);
        d.n = 0;
        off = 64;
        return R3D_OK;
    }
};
// Count of a compaction -- n flags and their exclusive scan -- which is the scan's last entry plus the last flag.  d_scan / d_flag
// are those two device words, for kernels enqueued before the host knows the count; add_to puts them into a read-back the caller
// owns, so whatever else it wants from the device (a bounding box, a deferred sort's test) travels in the same round trip.
struct CompactCount {
    const int *d_scan, *d_flag;
    int h_scan = 0, h_flag = 0;
    CompactCount(const int *scan, const int *flags, int64_t n) : d_scan(scan + (n - 1)), d_flag(flags + (n - 1)) {}
    int add_to(PinRead &rd) { if (int rc = rd.add(&h_scan, d_scan, 4)) return rc; return rd.add(&h_flag, d_flag, 4); }
    int64_t count() const { return (int64_t)h_scan + h_flag; }   // after the read-back's wait()
};

// means of the members `ld` loads through the index list: voxels up to VM_BIG members by a thread each, the listed rest by a wave
// each; scratch: (nseg + 16) ints (the counter, then the list)
template <class T, class LD>
static inline int launch_voxel_mean_ld(r3d_ctx *ctx, DevArena &ar, LD ld, const int *idx, const int *starts, int64_t nseg, int64_t n, double *out) {
    int *ws = (int *)ar.get((size_t)(nseg + 16) * 4);
    if (ar.rc) return ar.rc;
    R3D_HIP(ctx, hipMemsetAsync(ws, 0, 64, ctx->stream));
    const unsigned nb = (unsigned)((nseg + 255) / 256);
    const unsigned nbig = (unsigned)std::min<int64_t>(nseg, 4096);
    k_voxel_mean_t<T, LD><<<nb, 256, 0, ctx->stream>>>(ld, idx, starts, nseg, n, out, ws + 16, ws);
    k_voxel_mean_big<T, LD><<<nbig, 64, 0, ctx->stream>>>(ld, idx, starts, nseg, n, out, ws + 16, ws);
    R3D_HIP(ctx, hipGetLastError());
    return R3D_OK;
}
static inline int launch_voxel_mean(r3d_ctx *ctx, DevArena &ar, bool f32, const double *a, const int *idx, const int *starts, int64_t nseg, int64_t n,
                                    double *out, const double *sorted = nullptr) {
    if (sorted) {   // `a` in sorted order is available (the sort wrote it): contiguous streams, no index list
        const unsigned nbs = (unsigned)((nseg + 255) / 256);
        // R = 8 members per round trip: 4 / 8 / 16 measured 4.71 / 4.54-4.59 / 4.59-4.64 ms per C5 view, interleaved on one box
        if (f32) k_voxel_mean_sorted<float, 8><<<nbs, 256, 0, ctx->stream>>>(sorted, starts, nseg, n, out);
        else k_voxel_mean_sorted<double, 8><<<nbs, 256, 0, ctx->stream>>>(sorted, starts, nseg, n, out);
        R3D_HIP(ctx, hipGetLastError());
        return R3D_OK;
    }
    if (f32) return launch_voxel_mean_ld<float>(ctx, ar, MemberXyz{a}, idx, starts, nseg, n, out);
    return launch_voxel_mean_ld<double>(ctx, ar, MemberXyz{a}, idx, starts, nseg, n, out);
}

// Sorted cell keys are 32-bit whenever the key space allows, else 64-bit: calls the generic `f` with the pointer in its real type
// (where the keys are yet to be made, a null one: `decltype(+*k)` is the key type).
template <class F>
static inline auto with_keys(bool keys32, const void *keys, F &&f) {
    return keys32 ? f((const unsigned *)keys) : f((const unsigned long long *)keys);
}
// A run-time value as a template argument: calls the generic `f` with std::integral_constant<int, V> for the first V of the list
// that equals v, with the last one if none does
template <int V, int... Vs, class F>
static inline void with_const(int v, F &&f) {
    if constexpr (sizeof...(Vs) > 0) {
        if (v != V) return with_const<Vs...>(v, f);
    }
    f(std::integral_constant<int, V>{});
}

struct Grid {
    GridView v;
    int64_t n = 0;
    int64_t ncells = 0;
    void *keys = nullptr;   // sorted keys: unsigned if keys32, else unsigned long long
    bool keys32 = false;
    double mn[3], mx[3];
};

// a point at infinity (e.g. a zero disparity reprojected through Q) or a NaN has no cell: refuse instead of building a grid
// around it (fmin/fmax drop NaNs, so those show up as an untouched +-1e300 bound only if every value is NaN)
int bbox_check(r3d_ctx *ctx, const double mn[3], const double mx[3]) {
    for (int a = 0; a < 3; a++)
        if (!std::isfinite(mn[a]) || !std::isfinite(mx[a]) || mn[a] > mx[a] || std::fabs(mn[a]) > 1e290 || std::fabs(mx[a]) > 1e290)
            return r3d_fail(ctx, R3D_E_BADARG, "cloud has non-finite coordinates (axis %d spans [%g, %g])", a, mn[a], mx[a]);
    return R3D_OK;
}
// enqueues the bounding box of the first (*c0 + *c1) points (at most `bound`) and returns where its 6 doubles will be: the caller
// reads them with its next read-back, together with the count
int cloud_bbox_enqueue_dn(r3d_ctx *ctx, DevArena &ar, const double *d_pts, int64_t bound, const int *c0, const int *c1, const double **d_box6,
                          double *d_dst6 = nullptr /* where to leave the box (a buffer that outlives the arena); default: arena */) {
    const int nb = (int)std::min<int64_t>((bound + 255) / 256, 1024);
    double *part = (double *)ar.get((size_t)(nb + 1) * 6 * 8);
    if (ar.rc) return ar.rc;
    if (c0) k_bbox_partial_dn<<<nb, 256, 0, ctx->stream>>>(d_pts, c0, c1, part);
    else k_bbox_partial<<<nb, 256, 0, ctx->stream>>>(d_pts, bound, part);       // the count is known: `bound` IS the count
    double *dst = d_dst6 ? d_dst6 : part + (size_t)nb * 6;
    k_bbox_final<<<1, 256, 0, ctx->stream>>>(part, nb, dst);
    R3D_HIP(ctx, hipGetLastError());
    if (d_box6) *d_box6 = dst;
    return R3D_OK;
}
// an extra item for somebody else's read-back (PinRead): a value the caller wants on the host, produced earlier on the device
struct PinExtra { void *host = nullptr; const void *dev = nullptr; size_t bytes = 0; };
int cloud_bbox(r3d_ctx *ctx, DevArena &ar, const double *d_pts, int64_t n, double mn[3], double mx[3]) {
    const int nb = (int)std::min<int64_t>((n + 255) / 256, 1024);
    double *part = (double *)ar.get((size_t)(nb + 1) * 6 * 8);
    if (ar.rc) return ar.rc;
    k_bbox_partial<<<nb, 256, 0, ctx->stream>>>(d_pts, n, part);
    k_bbox_final<<<1, 256, 0, ctx->stream>>>(part, nb, part + (size_t)nb * 6);
    R3D_HIP(ctx, hipGetLastError());
    double h[6];
    {
        PinRead rd(ctx);
        int prc;
        if ((prc = rd.add(h, part + (size_t)nb * 6, sizeof h)) || (prc = rd.wait())) return prc;
    }
    for (int a = 0; a < 3; a++) { mn[a] = h[a]; mx[a] = h[3 + a]; }
    return bbox_check(ctx, mn, mx);
}

// exclusive scan of n ints / packed 64-bit counters on the ctx stream (k_scan_sums + k_scan_apply)
template <class T, bool MAXOP = false>
int dev_exclusive_scan(r3d_ctx *ctx, DevArena &ar, const T *in, T *out, int64_t n, int *lo_out = nullptr, int *hi_max = nullptr,
                       T *part = nullptr /* room for one T per SCAN_TILE elements, if the caller keeps one; default: from the arena */) {
    if (n <= 0) return R3D_OK;
    const int tiles = (int)((n + SCAN_TILE - 1) / SCAN_TILE);
    if (!part) part = (T *)ar.get((size_t)tiles * sizeof(T));
    if (ar.rc) return ar.rc;
    k_scan_sums<T, MAXOP><<<tiles, SCAN_T, 0, ctx->stream>>>(in, n, part);
    k_scan_apply<T, MAXOP><<<tiles, SCAN_T, 0, ctx->stream>>>(in, n, part, out, lo_out, hi_max);
    R3D_HIP(ctx, hipGetLastError());
    return R3D_OK;
}

// ---- stable LSD radix sort of (key, index) pairs, hand-written (rounds 1-3 called hipCUB here).  8 bits per pass; a pass is
// k_rx_hist (per-tile digit histogram) -> exclusive scan of the [256][tiles] table (digit-major: all tiles of digit 0, then digit
// 1, ...) -> k_rx_scatter (every item to scanned base of its (digit, tile) + its rank among the tile's items of that digit in
// original order).  A tile is ONE wave x 16 items, walked 64 items at a time: an item's rank inside such a group is the number of
// lower lanes holding the same digit -- eight ballots give every lane the mask of its peers -- plus a running per-digit count in
// LDS that the group's first peer advances; no cross-wave ordering to arrange, and the order is the stable one by construction.
// No host round trip, no fallback: used for cell sorts of large clouds without run structure (search-grid / Morton keys of an
// arbitrary cloud, where every point is its own run and the counting sort above degenerates to sorting runs one by one) and
// wherever the counting sort declines.
constexpr int RX_ITEMS = 16, RX_TILE = 64 * RX_ITEMS;
template <class KEY>
__global__ void __launch_bounds__(64) k_rx_hist(const KEY *__restrict__ keys, int64_t n, int shift, int *__restrict__ hist, int ntiles) {
    __shared__ int cnt[256];
    const int lane = threadIdx.x;
    for (int d = lane; d < 256; d += 64) cnt[d] = 0;
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * RX_TILE;
#pragma unroll
    for (int j = 0; j < RX_ITEMS; j++) {
        const int64_t i = base + j * 64 + lane;
        if (i < n) atomicAdd(&cnt[(int)((keys[i] >> shift) & 255)], 1);
    }
    __syncthreads();
    for (int d = lane; d < 256; d += 64) hist[(size_t)d * ntiles + blockIdx.x] = cnt[d];
}
template <class KEY, bool FIRST>
__global__ void __launch_bounds__(64) k_rx_scatter(const KEY *__restrict__ kin, const int *__restrict__ vin, int64_t n, int shift,
                                                   const int *__restrict__ offs, int ntiles, KEY *__restrict__ kout, int *__restrict__ vout) {
    __shared__ int base[256];
    const int lane = threadIdx.x;
    for (int d = lane; d < 256; d += 64) base[d] = offs[(size_t)d * ntiles + blockIdx.x];
    __syncthreads();
    const int64_t t0 = (int64_t)blockIdx.x * RX_TILE;
    const unsigned long long lt = lane == 0 ? 0ull : (~0ull >> (64 - lane));      // lanes below this one
    for (int j = 0; j < RX_ITEMS; j++) {
        const int64_t i = t0 + j * 64 + lane;
        const bool live = i < n;
        const KEY key = live ? kin[i] : (KEY)0;
        const int val = FIRST ? (int)i : (live ? vin[i] : 0);
        const int d = (int)((key >> shift) & 255);
        unsigned long long peers = __ballot(live);                                  // live lanes with my digit
#pragma unroll
        for (int b = 0; b < 8; b++) {
            const unsigned long long m = __ballot(live && ((d >> b) & 1));
            peers &= ((d >> b) & 1) ? m : ~m;
        }
        const int rank = __popcll(peers & lt), group = __popcll(peers);
        int pos = 0;
        if (live) pos = base[d] + rank;
        __syncthreads();                          // every lane has read its digit's count before the first peer advances it
        if (live && rank == 0) base[d] += group;
        __syncthreads();
        if (live) { kout[pos] = key; vout[pos] = val; }
    }
}

// sorts (cell key, index) pairs with the hand-written radix sort; keys come from k_cell_keys
template <class KEY>
int radix_sort_by_cell_t(r3d_ctx *ctx, DevArena &ar, const double *d_pts, int64_t n, const double org[3], double cell, const int dims[3],
                         int key_order, int bits, void **keys_sorted, int **idx_sorted) {
    KEY *k0 = (KEY *)ar.get((size_t)n * sizeof(KEY)), *k1 = (KEY *)ar.get((size_t)n * sizeof(KEY));
    int *v0 = (int *)ar.get((size_t)n * 4), *v1 = (int *)ar.get((size_t)n * 4);
    const int ntiles = (int)((n + RX_TILE - 1) / RX_TILE);
    int *hist = (int *)ar.get((size_t)256 * ntiles * 4), *offs = (int *)ar.get((size_t)256 * ntiles * 4);
    if (ar.rc) return ar.rc;
    const int nb = (int)((n + 255) / 256);
    k_cell_keys<KEY><<<nb, 256, 0, ctx->stream>>>(d_pts, n, org[0], org[1], org[2], cell, dims[0], dims[1], dims[2], key_order, k0, v0);
    R3D_HIP(ctx, hipGetLastError());
    const int passes = std::max(1, (bits + 7) / 8);
    KEY *kin = k0, *kout = k1;
    int *vin = v0, *vout = v1;
    for (int ps = 0; ps < passes; ps++) {
        k_rx_hist<KEY><<<ntiles, 64, 0, ctx->stream>>>(kin, n, 8 * ps, hist, ntiles);
        if (int rc = dev_exclusive_scan<int>(ctx, ar, hist, offs, (int64_t)256 * ntiles)) return rc;
        k_rx_scatter<KEY, false><<<ntiles, 64, 0, ctx->stream>>>(kin, vin, n, 8 * ps, offs, ntiles, kout, vout);   // (k_cell_keys wrote vals = index)
        R3D_HIP(ctx, hipGetLastError());
        std::swap(kin, kout);
        std::swap(vin, vout);
    }
    *keys_sorted = kin;
    *idx_sorted = vin;
    return R3D_OK;
}

constexpr int CS_MAX_RUNS = 4096;          // runs per bucket above which k_cs_rank's quadratic step is declined (radix fallback)
constexpr int64_t CS_MAX_BUCKETS = 1ll << 26;
// A sort whose host round trip (run count + fallback test) is DEFERRED: the caller adds d_total / d_maxruns to its own next
// read-back (PinRead) and calls ok(); if that says no, the sorted arrays are garbage and the caller sorts again with impl = 1.
struct SortDefer {
    const unsigned long long *d_total = nullptr;   // runs << 32 | points
    const int *d_maxruns = nullptr;
    int64_t n = 0;
    bool used = false;                             // false: the sort that ran was complete on its own (radix path)
    unsigned long long h_total = 0;
    int h_maxruns = 0;
    int add_to(PinRead &rd) { if (!used) return R3D_OK; if (int rc = rd.add(&h_total, d_total, 8)) return rc; return rd.add(&h_maxruns, d_maxruns, 4); }
    bool ok() const { return !used || (h_maxruns <= CS_MAX_RUNS && (int64_t)(unsigned)h_total == n); }
};
// returns R3D_OK with *done = false when it declines (more than CS_MAX_RUNS runs in one bucket)
template <class KEY>
int counting_sort_by_cell_t(r3d_ctx *ctx, DevArena &ar, const double *d_pts, int64_t n, const CsGeom &g, int64_t nbuckets, void **keys_sorted,
                            int **idx_sorted, double *sorted_pts, bool *done, SortDefer *defer = nullptr) {
    *done = false;
    KEY *keys = (KEY *)ar.get((size_t)n * sizeof(KEY)), *keys_out = (KEY *)ar.get((size_t)n * sizeof(KEY));
    int *gid_of = (int *)ar.get((size_t)n * 4), *idx_out = (int *)ar.get((size_t)n * 4), *final_base = (int *)ar.get((size_t)n * 4);
    CsRun<KEY> *runs = (CsRun<KEY> *)ar.get((size_t)n * sizeof(CsRun<KEY>)), *placed = (CsRun<KEY> *)ar.get((size_t)n * sizeof(CsRun<KEY>));
    // bucket table (nbuckets + 1 entries, the last one stays 0) followed by the counter cell: ONE fill zeroes both
    unsigned long long *cnt = (unsigned long long *)ar.get((size_t)(nbuckets + 1 + 8) * 8), *start = (unsigned long long *)ar.get((size_t)(nbuckets + 1) * 8);
    if (ar.rc) return ar.rc;
    int *ctr = (int *)(cnt + nbuckets + 1);   // [0] most runs in one bucket
    R3D_HIP(ctx, hipMemsetAsync(cnt, 0, (size_t)(nbuckets + 1 + 8) * 8, ctx->stream));
    const int nb = (int)((n + 255) / 256);
    k_cs_runs<KEY><<<nb, 256, 0, ctx->stream>>>(d_pts, n, g, keys, gid_of, cnt, runs);
    int rc = dev_exclusive_scan<unsigned long long>(ctx, ar, cnt, start, nbuckets + 1, nullptr, ctr);
    if (rc) return rc;
    if (defer) {   // no round trip here: launch over the upper bounds, counts and the fallback test stay on the device for now
        k_cs_place<KEY><<<nb, 256, 0, ctx->stream>>>(runs, gid_of, n, start, placed);
        k_cs_rank<KEY><<<nb, 256, 0, ctx->stream>>>(placed, 0, start, final_base, start + nbuckets, ctr, CS_MAX_RUNS);
        k_cs_emit<KEY><<<nb, 256, 0, ctx->stream>>>(keys, gid_of, final_base, n, keys_out, idx_out, d_pts, sorted_pts, ctr, CS_MAX_RUNS);
        R3D_HIP(ctx, hipGetLastError());
        defer->d_total = start + nbuckets;
        defer->d_maxruns = ctr;
        defer->n = n;
        defer->used = true;
        *keys_sorted = keys_out;
        *idx_sorted = idx_out;
        *done = true;
        return R3D_OK;
    }
    // ONE host round trip: the scan total (runs << 32 | points: cnt[nbuckets] is 0, so start[nbuckets] is the total) and the
    // largest run count of a bucket, which decides whether the quadratic ranking step is affordable
    struct { unsigned long long total; int max_runs; } h = {0, 0};
    {
        PinRead rd(ctx);
        int prc;
        if ((prc = rd.add(&h.total, start + nbuckets, 8)) || (prc = rd.add(&h.max_runs, ctr, 4)) || (prc = rd.wait())) return prc;
    }
    if ((int64_t)(unsigned)h.total != n) return r3d_fail(ctx, R3D_E_HIP, "counting sort: bucket populations sum to %u, expected %lld", (unsigned)h.total, (long long)n);
    static const bool dbg = [] { const char *e = getenv("R3D_SORT_DEBUG"); return e && *e == '1'; }();
    if (dbg) fprintf(stderr, "[r3d sort] n=%lld key_order=%d buckets=%lld runs=%d max_runs_per_bucket=%d keys%d\n", (long long)n, g.key_order,
                     (long long)nbuckets, (int)(h.total >> 32), h.max_runs, (int)sizeof(KEY) * 8);
    if (h.max_runs > CS_MAX_RUNS) return R3D_OK;
    const int nruns = (int)(h.total >> 32), nrb = (nruns + 255) / 256;
    k_cs_place<KEY><<<nb, 256, 0, ctx->stream>>>(runs, gid_of, n, start, placed);
    k_cs_rank<KEY><<<nrb, 256, 0, ctx->stream>>>(placed, nruns, start, final_base, nullptr, nullptr, 0);
    k_cs_emit<KEY><<<nb, 256, 0, ctx->stream>>>(keys, gid_of, final_base, n, keys_out, idx_out, d_pts, sorted_pts, nullptr, 0);
    R3D_HIP(ctx, hipGetLastError());
    *keys_sorted = keys_out;
    *idx_sorted = idx_out;
    *done = true;
    return R3D_OK;
}

// sorts point indices by (cell key, index); fills keys_sorted / idx_sorted (device) and, if sorted_pts != NULL, the points in that
// order.  The keys are 32-bit whenever the key space allows; *keys32 tells the caller which type keys_sorted points to.
// Default: the run-based counting sort above; the library radix sort when that declines.
int sort_by_cell(r3d_ctx *ctx, DevArena &ar, const double *d_pts, int64_t n, const double org[3], double cell, const int dims[3],
                 int key_order, void **keys_sorted, bool *keys32, int **idx_sorted, double *sorted_pts = nullptr, int impl = -1,
                 SortDefer *defer = nullptr) {
    if (defer) *defer = SortDefer();
    int bits = 1;
    if (key_order == 2) {
        int m = std::max(dims[0], std::max(dims[1], dims[2])), b1 = 1;
        while ((1 << b1) < m) b1++;
        bits = std::min(63, 3 * b1);
    } else {
        const unsigned long long maxkey = (unsigned long long)dims[0] * dims[1] * dims[2];
        while (bits < 64 && (maxkey >> bits)) bits++;
    }
    *keys32 = bits <= 32;
    static const int env_impl = [] { const char *e = getenv("R3D_SORT_IMPL"); return !e ? -1 : !strcmp(e, "radix") ? 1 : !strcmp(e, "counting") ? 0 : -1; }();
    // default choice: the counting sort where keys arrive in runs (voxel keys of image- or voxel-ordered clouds) and for small
    // clouds (six launches + one round trip); the radix sort for search-grid / Morton keys of large clouds, which have no run
    // structure to exploit (every point its own run: 1 M points 0.19 ms against 0.09 ms, and no host round trip)
    static const int64_t rx_min = [] { const char *e = getenv("R3D_SORT_RADIX_MIN"); return e ? (int64_t)atoll(e) : (int64_t)262144; }();
    const bool prefer_radix = (key_order == 0 || key_order == 2) && n >= rx_min;
    const bool force_radix = impl >= 0 ? impl == 1 : (env_impl >= 0 ? env_impl == 1 : prefer_radix);
    // bucket table of the counting sort: a monotone coarsening of the key (consecutive keys share a bucket) with about half as
    // many entries as there are points (2^14 .. 2^26): small enough to fill and scan in a few microseconds, fine enough that a
    // bucket holds tens of runs (the ranking step is quadratic in the runs of a bucket: whole (kx, ky) columns of an 8 MP view,
    // pierced lengthwise by a slanted surface, held up to 1 500)
    CsGeom g{org[0], org[1], org[2], cell, dims[0], dims[1], dims[2], key_order, 0, 1};
    int64_t nbuckets;
    int tb = 14;
    // voxel keys of image-ordered clouds arrive in runs of several points (n / 2 buckets); search-grid and Morton keys of an
    // unordered cloud are one run per point, so the ranking step wants few points per bucket (2 n buckets)
    const int64_t want = (key_order == 1 || key_order == 3) ? n / 2 : 2 * n;
    while (tb < 26 && (1ll << tb) < want) tb++;
    if (key_order == 1 || key_order == 3) {
        const long double total = (long double)dims[0] * dims[1] * dims[2];
        unsigned long long d = (unsigned long long)(total / (long double)(1ll << tb)) + 1;
        g.shift = -1;
        g.div = d;
        nbuckets = (int64_t)(total / (long double)d) + 2;
    } else {
        g.shift = std::max(0, bits - tb);
        nbuckets = key_order == 2 ? (1ll << (bits - g.shift)) : (int64_t)(((unsigned long long)dims[0] * dims[1] * dims[2]) >> g.shift) + 1;
    }
    if (!force_radix && nbuckets <= CS_MAX_BUCKETS && n < 0x7fffffff) {
        bool done = false;
        const int rc = with_keys(*keys32, nullptr, [&](auto *k) {
            return counting_sort_by_cell_t<decltype(+*k)>(ctx, ar, d_pts, n, g, nbuckets, keys_sorted, idx_sorted, sorted_pts, &done, defer);
        });
        if (rc || done) return rc;
    }
    const int rc = with_keys(*keys32, nullptr, [&](auto *k) {
        return radix_sort_by_cell_t<decltype(+*k)>(ctx, ar, d_pts, n, org, cell, dims, key_order, bits, keys_sorted, idx_sorted);
    });
    if (rc) return rc;
    if (sorted_pts) {
        k_gather3<<<(unsigned)((n + 255) / 256), 256, 0, ctx->stream>>>(d_pts, *idx_sorted, n, sorted_pts);
        R3D_HIP(ctx, hipGetLastError());
    }
    return R3D_OK;
}

// Builds the search grid.  cell_hint: minimum useful cell (search radius, or <= 0 for pure kNN); the cell is
// refined so that occupied cells hold about `target_occ` points, and coarsened to keep the dense table <= 2^26 cells.
// enclosing[6] (optional): a box known to contain every point (e.g. the bounding box of the cloud these points are voxel means
// of): used, slightly widened, instead of a bounding-box pass and its host round trip.  A search grid's origin and extent decide
// only which cell a point is filed under; what the searches return does not depend on them.
// spacing_hint (optional): the cloud is a voxel-down-sampled surface with this voxel size, so a cell of side c holds about
// (c / spacing)^2 points -- used instead of the bounding-box estimate below, which is off by 3-6x on a room-sized scan (the box's
// faces are not the surface) and then picks cells of HALF the correspondence radius: every query whose nearest point is further
// than one such cell -- most of them while a scan frame is still misaligned by a centimetre -- walks the 98 cells of shell 2.
int grid_build(r3d_ctx *ctx, DevArena &ar, const double *d_pts, int64_t n, double cell_hint, double target_occ, Grid &G, bool dense_table = false,
               const double *enclosing = nullptr, double spacing_hint = 0) {
    if (n <= 0) return r3d_fail(ctx, R3D_E_BADARG, "grid: empty cloud");
    if (n > 0x7fffffff) return r3d_fail(ctx, R3D_E_UNSUPPORTED, "grid: more than 2^31-1 points");
    int rc;
    if (enclosing) {
        for (int a = 0; a < 3; a++) {   // a mean of values inside [lo, hi] can leave it by a rounding: widen by far more than that
            const double pad = 1e-9 * std::max(std::max(std::fabs(enclosing[a]), std::fabs(enclosing[3 + a])), enclosing[3 + a] - enclosing[a]) + 1e-300;
            G.mn[a] = enclosing[a] - pad;
            G.mx[a] = enclosing[3 + a] + pad;
        }
        if ((rc = bbox_check(ctx, G.mn, G.mx))) return rc;
    } else if ((rc = cloud_bbox(ctx, ar, d_pts, n, G.mn, G.mx))) return rc;
    double ext[3];
    for (int a = 0; a < 3; a++) ext[a] = std::max(G.mx[a] - G.mn[a], 1e-9);
    // surface-like data: occupied cells ~ (extent/cell)^2 * const.  Start from the volume / area heuristic and clamp.
    const double diag = std::sqrt(ext[0] * ext[0] + ext[1] * ext[1] + ext[2] * ext[2]);
    double cell = cell_hint > 0 ? cell_hint : diag / std::max(1.0, std::sqrt((double)n / std::max(target_occ, 1.0)));
    if (cell_hint > 0 && target_occ > 0) {
        // estimate occupancy at cell_hint assuming a 2-manifold: area ~ n * spacing^2, spacing from bbox area
        const double area = 2.0 * (ext[0] * ext[1] + ext[1] * ext[2] + ext[0] * ext[2]) / 2.0;  // rough
        const double per_cell = spacing_hint > 0 ? (cell_hint / spacing_hint) * (cell_hint / spacing_hint)
                                                 : (double)n * cell_hint * cell_hint / std::max(area, 1e-30);
        int m = (int)std::floor(std::sqrt(std::max(per_cell / target_occ, 1.0)));
        m = std::max(1, std::min(m, 16));
        cell = cell_hint / m;
    }
    int dims[3];
    for (;;) {
        double nc = 1;
        for (int a = 0; a < 3; a++) { dims[a] = (int)std::floor(ext[a] / cell) + 1; nc *= dims[a]; }
        if (nc <= (double)(1 << 26)) break;
        cell *= 1.26;
    }
    G.n = n;
    G.ncells = (int64_t)dims[0] * dims[1] * dims[2];
    int *idx;
    double *sorted = (double *)ar.get((size_t)n * 24);
    if (ar.rc) return ar.rc;
    rc = sort_by_cell(ctx, ar, d_pts, n, G.mn, cell, dims, 0, &G.keys, &G.keys32, &idx, sorted);   // writes the cell-sorted copy as well
    if (rc) return rc;
    // R3D_CELL_TABLE = dense | lines overrides the caller's choice (A/B)
    static const int table_env = [] { const char *e = getenv("R3D_CELL_TABLE"); return !e ? -1 : !strcmp(e, "dense") ? 1 : !strcmp(e, "lines") ? 0 : -1; }();
    if (table_env >= 0) dense_table = table_env == 1;
    if (dense_table) {
        int *cnt = (int *)ar.get((size_t)(G.ncells + 1) * 4), *rs = (int *)ar.get((size_t)(G.ncells + 1) * 4);
        int *cs = (int *)ar.get((size_t)(G.ncells + 1 + 4) * 4);   // + 4: the search reads 16 bytes at a run's first cell
        if (ar.rc) return ar.rc;
        R3D_HIP(ctx, hipMemsetAsync(cnt, 0, (size_t)(G.ncells + 1) * 4, ctx->stream));
        const int nbd = (int)((n + 255) / 256);
        with_keys(G.keys32, G.keys, [&](auto *keys) {
            k_cell_counts<<<nbd, 256, 0, ctx->stream>>>(keys, n, rs, cnt);
            k_cell_counts2<<<nbd, 256, 0, ctx->stream>>>(keys, n, rs, cnt);
        });
        if ((rc = dev_exclusive_scan<int>(ctx, ar, cnt, cs, G.ncells + 1))) return rc;
        G.v = GridView{G.mn[0], G.mn[1], G.mn[2], cell, 1.0 / cell, dims[0], dims[1], dims[2], nullptr, nullptr, cs, sorted, idx, nullptr};
        return R3D_OK;
    }
    // two-level cell table from the sorted keys (GridView::l1 / l2); sized for the worst case, only materialised lines are touched
    const int64_t nl = ((G.ncells + CL_STRIDE) >> CL_SHIFT) + 1;
    const int64_t max_lines = std::min<int64_t>(nl, 2 * n + 1);
    // one fill zeroes both; last1 starts at a multiple of four ints so that the scans' 16-byte accesses stay aligned
    const int64_t nl4 = (nl + 3) & ~(int64_t)3;
    int *mark = (int *)ar.get((size_t)(nl4 + nl) * 4), *last1 = mark + nl4;
    int *ids = (int *)ar.get((size_t)nl * 4), *before = (int *)ar.get((size_t)nl * 4), *l1 = (int *)ar.get((size_t)nl * 4);
    int *l2 = (int *)ar.get((size_t)(max_lines + 1) * CL_STRIDE * 4);
    if (ar.rc) return ar.rc;
    R3D_HIP(ctx, hipMemsetAsync(mark, 0, (size_t)(nl4 + nl) * 4, ctx->stream));
    const int nb = (int)((n + 255) / 256), nlb = (int)((nl + 255) / 256);
    with_keys(G.keys32, G.keys, [&](auto *keys) { k_line_mark<<<nb, 256, 0, ctx->stream>>>(keys, n, mark, last1); });
    if ((rc = dev_exclusive_scan<int>(ctx, ar, mark, ids, nl))) return rc;
    if ((rc = dev_exclusive_scan<int, true>(ctx, ar, last1, before, nl))) return rc;
    k_line_l1<<<nlb, 256, 0, ctx->stream>>>(mark, ids, before, nl, l1);
    with_keys(G.keys32, G.keys, [&](auto *keys) { k_line_fill<<<(unsigned)((n + 256) / 256), 256, 0, ctx->stream>>>(keys, n, l1, nl, l2); });
    R3D_HIP(ctx, hipGetLastError());
    G.v = GridView{G.mn[0], G.mn[1], G.mn[2], cell, 1.0 / cell, dims[0], dims[1], dims[2], l1, l2, nullptr, sorted, idx, nullptr};
    return R3D_OK;
}

Rigid to_rigid(const double T[16]) {
    Rigid r;
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) r.r[i * 3 + j] = T[i * 4 + j];
        r.t[i] = T[i * 4 + 3];
    }
    return r;
}
__host__ __device__ void mat4_mul(const double A[16], const double B[16], double C[16]) {
    double t[16];
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) {
            double s = 0;
            for (int k = 0; k < 4; k++) s += A[i * 4 + k] * B[k * 4 + j];
            t[i * 4 + j] = s;
        }
    for (int i = 0; i < 16; i++) C[i] = t[i];
}

// 3x3 SVD via Jacobi eigen-decomposition of S^T S (float64) -- only used for the 3x3 Kabsch/Umeyama step.  The update of a
// registration iteration (this, umeyama_from_sums, solve6_to_matrix) runs in one thread of k_icp_step.
__host__ __device__ void jacobi_eig3(double A[3][3], double V[3][3]) {
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) V[i][j] = i == j;
    // Cyclic Jacobi with the annihilated element set to exactly zero: the off-diagonal mass then falls quadratically to below
    // 1e-30 of the diagonal in 5-7 sweeps.  (Without the explicit zero the rounding residue of every rotation, ~1e-17 of the
    // diagonal, keeps all 60 sweeps busy: 72 us per step in one GPU thread, three times the evaluation kernel of a 40 k-point
    // cloud.)
    for (int sweep = 0; sweep < 60; sweep++) {
        const double off = fabs(A[0][1]) + fabs(A[0][2]) + fabs(A[1][2]), scale = fabs(A[0][0]) + fabs(A[1][1]) + fabs(A[2][2]);
        if (off < 1e-300 || off <= 1e-30 * scale) break;
        for (int p = 0; p < 2; p++)
            for (int q = p + 1; q < 3; q++) {
                if (fabs(A[p][q]) <= 1e-33 * scale) { A[p][q] = A[q][p] = 0; continue; }
                double theta = (A[q][q] - A[p][p]) / (2 * A[p][q]);
                double t = (theta >= 0 ? 1 : -1) / (fabs(theta) + sqrt(theta * theta + 1));
                double c = 1 / sqrt(t * t + 1), s = t * c;
                for (int k = 0; k < 3; k++) { double a = A[k][p], b = A[k][q]; A[k][p] = c * a - s * b; A[k][q] = s * a + c * b; }
                for (int k = 0; k < 3; k++) { double a = A[p][k], b = A[q][k]; A[p][k] = c * a - s * b; A[q][k] = s * a + c * b; }
                for (int k = 0; k < 3; k++) { double a = V[k][p], b = V[k][q]; V[k][p] = c * a - s * b; V[k][q] = s * a + c * b; }
                A[p][q] = A[q][p] = 0;
            }
    }
}
__host__ __device__ double det3(const double M[3][3]) {
    return M[0][0] * (M[1][1] * M[2][2] - M[1][2] * M[2][1]) - M[0][1] * (M[1][0] * M[2][2] - M[1][2] * M[2][0]) +
           M[0][2] * (M[1][0] * M[2][1] - M[1][1] * M[2][0]);
}
// Eigen::umeyama(src, dst, false) from the accumulated sums: returns U (4x4) mapping src -> dst.
// rank_tol: a singular value counts when it is above rank_tol x the largest.  They are roots of the eigenvalues of sigma^T sigma,
// whose rounding noise is ~1e-16 of the largest eigenvalue, i.e. up to ~5e-8 of the largest SINGULAR value: under a tolerance
// below that (the registration loop once passed 1e-14) an exactly deficient covariance (three pairs always are: rank 2; so is a
// wall) is taken for full rank whenever that noise comes out positive, and the left vector made from it is not orthogonal to the
// others.  Both callers pass 1e-6 (RANSAC_RANK_TOL, ICP_RANK_TOL) and follow with umeyama_polish.
// The means and products in `s` may be relative to any common origin: R does not depend on it, and the translation written
// here is the one between the relative frames (icp_p2p_update moves it back).
__host__ __device__ void umeyama_from_sums(const double *s /*ICP slots*/, double U[16], double rank_tol) {
    const double n = s[0];
    const double ps[3] = {s[2] / n, s[3] / n, s[4] / n}, pt[3] = {s[5] / n, s[6] / n, s[7] / n};
    double sigma[3][3];  // (1/n) sum (t - mt)(p - mp)^T  = E[t p^T] - mt mp^T ; slots hold p_i t_j
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) sigma[i][j] = s[8 + j * 3 + i] / n - pt[i] * ps[j];
    // SVD sigma = Us D Vs^T through the symmetric eigenproblems
    double StS[3][3], V[3][3];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) { StS[i][j] = 0; for (int k = 0; k < 3; k++) StS[i][j] += sigma[k][i] * sigma[k][j]; }
    jacobi_eig3(StS, V);
    // eigenvalues in descending order, eigenvectors with them: the stable insertion sort of three as its compare-and-swap network
    // (0,1) (1,2) (0,1) on VALUES -- an index permutation (V[r][ord[c]]) is a dynamically indexed local array, which the compiler
    // keeps in scratch memory: several dependent memory round trips in the one thread the whole loop waits for
    double ev[3] = {StS[0][0], StS[1][1], StS[2][2]};
    double Vs[3][3], Us[3][3], sv[3];
    for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) Vs[r][c] = V[r][c];
    auto cswap = [&](int a, int b) {   // a < b: swap when the later one is strictly larger (ties keep their order)
        if (ev[b] > ev[a]) {
            const double t = ev[a]; ev[a] = ev[b]; ev[b] = t;
            for (int r = 0; r < 3; r++) { const double u = Vs[r][a]; Vs[r][a] = Vs[r][b]; Vs[r][b] = u; }
        }
    };
    cswap(0, 1); cswap(1, 2); cswap(0, 1);
    for (int c = 0; c < 3; c++) sv[c] = sqrt(fmax(ev[c], 0.0));
    int rank = 0;   // singular values are in descending order: the deficient columns come last
    for (int c = 0; c < 3; c++) {
        double u[3] = {0, 0, 0};
        for (int r = 0; r < 3; r++) for (int k = 0; k < 3; k++) u[r] += sigma[r][k] * Vs[k][c];
        double l = sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
        if (!(l > 1e-300 && sv[c] > rank_tol * fmax(sv[0], 1e-300))) break;
        for (int r = 0; r < 3; r++) Us[r][c] = u[r] / l;
        rank = c + 1;
    }
    if (rank == 2) {          // planar correspondences: third left vector completes a right-handed basis
        Us[0][2] = Us[1][0] * Us[2][1] - Us[2][0] * Us[1][1];
        Us[1][2] = Us[2][0] * Us[0][1] - Us[0][0] * Us[2][1];
        Us[2][2] = Us[0][0] * Us[1][1] - Us[1][0] * Us[0][1];
    } else if (rank == 0) {   // one pair, or all pairs coincident: pure translation (an SVD of the zero matrix is U = V = I)
        for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) Us[r][c] = Vs[r][c];
    } else if (rank == 1) {   // collinear pairs: the twist about the line is undetermined; take the smallest rotation v0 -> u0
        const double v0[3] = {Vs[0][0], Vs[1][0], Vs[2][0]}, u0[3] = {Us[0][0], Us[1][0], Us[2][0]};
        const double cs = v0[0] * u0[0] + v0[1] * u0[1] + v0[2] * u0[2];
        double Rm[3][3];
        if (cs > -1 + 1e-12) {
            const double w[3] = {v0[1] * u0[2] - v0[2] * u0[1], v0[2] * u0[0] - v0[0] * u0[2], v0[0] * u0[1] - v0[1] * u0[0]};
            const double K[3][3] = {{0, -w[2], w[1]}, {w[2], 0, -w[0]}, {-w[1], w[0], 0}};
            for (int i = 0; i < 3; i++)
                for (int j = 0; j < 3; j++) {
                    double k2 = 0;
                    for (int k = 0; k < 3; k++) k2 += K[i][k] * K[k][j];
                    Rm[i][j] = (i == j) + K[i][j] + k2 / (1 + cs);
                }
        } else {                // opposite directions: half turn about the second right vector (orthogonal to v0)
            for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) Rm[i][j] = 2 * Vs[i][1] * Vs[j][1] - (i == j);
        }
        for (int c = 1; c < 3; c++)
            for (int r = 0; r < 3; r++) Us[r][c] = Rm[r][0] * Vs[0][c] + Rm[r][1] * Vs[1][c] + Rm[r][2] * Vs[2][c];
    }
    double S[3] = {1, 1, 1};
    if (det3(Us) * det3(Vs) < 0) S[2] = -1;
    double R[3][3];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) { R[i][j] = 0; for (int k = 0; k < 3; k++) R[i][j] += Us[i][k] * S[k] * Vs[j][k]; }
    for (int i = 0; i < 16; i++) U[i] = (i % 5 == 0);
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) U[i * 4 + j] = R[i][j];
        U[i * 4 + 3] = pt[i] - (R[i][0] * ps[0] + R[i][1] * ps[1] + R[i][2] * ps[2]);
    }
}

// Newton steps on the rotation umeyama_from_sums returned, for RANSAC's 3-4 pair samples.  That routine goes through the eigenvectors
// of sigma^T sigma, so its rotation is off by ~2e-17 (sigma_1 / sigma_2)^2: 2e-9 for a sample whose second singular value is 1e-4
// of the first (measured against an SVD).  The least-squares rotation R makes R^T sigma symmetric; with A = R^T sigma, S its
// symmetric part and R <- R exp([w]x), the first-order condition is (tr(S) I - S) w = vee(A - A^T), a 3x3 system whose smallest
// eigenvalue is sigma_2 + sigma_3: conditioning linear in sigma_1 / sigma_2, and the step converges quadratically from a start that
// close.  Skipped when that system is singular to 1e-8 (rank <= 1: the routine's defined answer stays) or the step is not small.
__host__ __device__ void umeyama_polish(const double *s /*ICP slots*/, double U[16]) {
    const double n = s[0];
    const double ps[3] = {s[2] / n, s[3] / n, s[4] / n}, pt[3] = {s[5] / n, s[6] / n, s[7] / n};
    double sg[3][3], R[3][3];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) { sg[i][j] = s[8 + j * 3 + i] / n - pt[i] * ps[j]; R[i][j] = U[i * 4 + j]; }
    {   // the routine's third left vector comes from sigma v3 / |sigma v3|, which a tiny sigma_3 leaves ~1e-16 sigma_1^2 / (sigma_2 sigma_3) off
        // the others' orthogonal complement (3e-11 seen): one Newton-Schulz step R <- R (3 I - R^T R) / 2 squares that away
        double G[3][3], Rn[3][3];
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) G[i][j] = 3.0 * (i == j) - ((R[0][i] * R[0][j] + R[1][i] * R[1][j]) + R[2][i] * R[2][j]);
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) Rn[i][j] = 0.5 * ((R[i][0] * G[0][j] + R[i][1] * G[1][j]) + R[i][2] * G[2][j]);
        for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) R[i][j] = Rn[i][j];
    }
    for (int it = 0; it < 2; it++) {
        double A[3][3];
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) A[i][j] = (R[0][i] * sg[0][j] + R[1][i] * sg[1][j]) + R[2][i] * sg[2][j];
        const double a[3] = {A[2][1] - A[1][2], A[0][2] - A[2][0], A[1][0] - A[0][1]};
        const double tr = A[0][0] + A[1][1] + A[2][2];
        const double m00 = tr - A[0][0], m11 = tr - A[1][1], m22 = tr - A[2][2];
        const double m01 = -0.5 * (A[0][1] + A[1][0]), m02 = -0.5 * (A[0][2] + A[2][0]), m12 = -0.5 * (A[1][2] + A[2][1]);
        const double c00 = m11 * m22 - m12 * m12, c01 = m02 * m12 - m01 * m22, c02 = m01 * m12 - m02 * m11;
        const double c11 = m00 * m22 - m02 * m02, c12 = m01 * m02 - m00 * m12, c22 = m00 * m11 - m01 * m01;
        const double det = (m00 * c00 + m01 * c01) + m02 * c02;
        if (!(tr > 0.0 && det > 1e-8 * tr * tr * tr)) break;
        const double w[3] = {((c00 * a[0] + c01 * a[1]) + c02 * a[2]) / det, ((c01 * a[0] + c11 * a[1]) + c12 * a[2]) / det,
                             ((c02 * a[0] + c12 * a[1]) + c22 * a[2]) / det};
        const double th2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2];
        if (!(th2 < 1e-6)) break;
        const double f1 = 1.0 - th2 / 6.0, f2 = 0.5 - th2 / 24.0;       // sin(t) / t and (1 - cos(t)) / t^2 to below 1e-14 here
        const double K[3][3] = {{0, -w[2], w[1]}, {w[2], 0, -w[0]}, {-w[1], w[0], 0}};
        double E[3][3], Rn[3][3];
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++)
                E[i][j] = ((i == j) + f1 * K[i][j]) + f2 * ((K[i][0] * K[0][j] + K[i][1] * K[1][j]) + K[i][2] * K[2][j]);
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) Rn[i][j] = (R[i][0] * E[0][j] + R[i][1] * E[1][j]) + R[i][2] * E[2][j];
        for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) R[i][j] = Rn[i][j];
    }
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) U[i * 4 + j] = R[i][j];
        U[i * 4 + 3] = pt[i] - (R[i][0] * ps[0] + R[i][1] * ps[1] + R[i][2] * ps[2]);
    }
}

// One step of the registration loop on the device.  16 waves: wave w reduces slots w and w + 16 (lane t adds the partials
// t, t+64, ... in order, then a fixed shuffle tree => deterministic); thread 0 then does what the host loop of
// RegistrationICP does between two evaluations: statistics, convergence test against the previous evaluation, update
// (Umeyama or the 6x6 Gauss-Newton system) and T <- U T.
// `mirror` (pinned host memory, device-visible): thread 0 publishes the state there after every step, fields first, then a
// system-scope fence, then `seq`; the host polls `seq` / `done` in that memory instead of waiting for a copy and an event -- the
// completion of a D2H copy + marker reached the host 16-57 ms late about once in 16 registrations of 1 M points (the device clock
// in the state showed the device done on time: R3D_ICP_DEBUG), a kernel's own store does not go that way.
__device__ __forceinline__ void icp_publish(const IcpState *st, IcpState *mirror) {
    if (!mirror) return;
    for (int i = 0; i < 16; i++) mirror->T[i] = st->T[i];
    mirror->fit = st->fit; mirror->rmse = st->rmse; mirror->corr = st->corr;
    mirror->evals = st->evals; mirror->converged = st->converged; mirror->iterations = st->iterations;
    mirror->t_first = st->t_first; mirror->t_last = st->t_last;
    mirror->done = st->done;
    __threadfence_system();
    // the termination travels in the released word itself: a plain `done` store could become visible before the statistics
    // above, and the host would copy a stale iteration count / fitness (the fields share one 64-byte line)
    *(volatile int *)&mirror->seq = st->evals | (st->done ? ICP_SEQ_DONE : 0);
}
// The reduction of k_icp_eval's partial sums, by a 1024-thread workgroup: 16 waves, wave w reduces slots w and w + 16 into
// sums[]; the caller places the barrier.  k_icp_step and the read-out of r3d_debug_icp_sums share it.
__device__ __forceinline__ void icp_reduce_partials(const double *__restrict__ partial, int nblocks, double *sums /* shared, [32] */) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    // wave w owns slots w and w + 16; the partial sums are stored [slot][workgroup], so lane t reads t, t + 64, ... of a
    // contiguous run, twelve requests per slot in flight (768 workgroups = one round), added in ascending order: the same
    // sum, bit for bit, as one lane walking them one dependent load at a time (that walk was 2 x 12 L2 round trips of the
    // 12 us this kernel took)
    constexpr int U = 12;
    const int s0 = w, s1 = w + 16;
    const bool two = s1 < ICP_SLOTS;
    const double *p0 = partial + (size_t)s0 * nblocks, *p1 = partial + (size_t)(two ? s1 : s0) * nblocks;
    double v0 = 0, v1 = 0;
    for (int b0 = 0; b0 < nblocks; b0 += 64 * U) {
        double a0[U], a1[U];
#pragma unroll
        for (int j = 0; j < U; j++) {
            const int b = b0 + j * 64 + lane, bc = min(b, nblocks - 1);   // clamped address + select: no branch around a load
            const double x0 = p0[bc], x1 = p1[bc];
            a0[j] = b < nblocks ? x0 : 0.0;
            a1[j] = b < nblocks ? x1 : 0.0;
        }
#pragma unroll
        for (int j = 0; j < U; j++) { v0 += a0[j]; v1 += a1[j]; }
    }
    v0 = wave_sum(v0);
    v1 = wave_sum(v1);
    if (lane == 0) { sums[s0] = v0; if (two) sums[s1] = v1; }
}

// r3d_debug_icp_sums: the 29 slots of one evaluation as k_icp_step would see them (its reduction, nothing else)
__global__ void __launch_bounds__(1024) k_icp_sums_readout(const double *__restrict__ partial, int nblocks, double *__restrict__ out) {
    __shared__ double sums[32];
    icp_reduce_partials(partial, nblocks, sums);
    __syncthreads();
    if (threadIdx.x < ICP_SLOTS) out[threadIdx.x] = sums[threadIdx.x];
}

// The point-to-point update from the slots k_icp_eval accumulates relative to the origin o (the centre of the target grid's
// box): Umeyama on the relative moments, then the translation back in world coordinates, t = (o + mu) - R (o + mq) with mq, mu
// the relative means.
// The rank rule is RANSAC's (see umeyama_from_sums): walls and floors give rank-2 covariances, whose third singular value is
// rounding noise; under the 1e-14 this loop used to pass that noise counted as a direction and the rotation came out
// non-orthonormal (1e-3 on a flat patch).  umeyama_polish then takes the rotation from the eigenvector route's ~1e-13 to the
// least-squares rotation of sigma itself.
// The translation is summed in double-double (error-free products and sums, one rounding at the end): its terms are as large
// as the clouds' distance from the world origin, the result as small as the motion, and a plain sum would round at the former.
constexpr double ICP_RANK_TOL = 1e-6;
__host__ __device__ inline void dd_add(double &hi, double &lo, double x) {   // (hi, lo) += x, hi + lo exact to the sum's second order
    const double s = hi + x, b = s - hi;
    lo += (hi - (s - b)) + (x - b);
    hi = s;
}
__host__ __device__ void icp_p2p_update(const double *sums, const IcpOrigin &org, double U[16]) {
    umeyama_from_sums(sums, U, ICP_RANK_TOL);
    umeyama_polish(sums, U);
    const double n = sums[0], o[3] = {org.x, org.y, org.z};
    const double mq[3] = {sums[2] / n, sums[3] / n, sums[4] / n}, mu[3] = {sums[5] / n, sums[6] / n, sums[7] / n};
    for (int i = 0; i < 3; i++) {
        double hi = o[i], lo = 0;
        dd_add(hi, lo, mu[i]);
        for (int j = 0; j < 3; j++) {
            const double r = -U[i * 4 + j];
            const double a = r * o[j], b = r * mq[j];
            lo += fma(r, o[j], -a) + fma(r, mq[j], -b);   // what the two products rounded away
            dd_add(hi, lo, a);
            dd_add(hi, lo, b);
        }
        U[i * 4 + 3] = hi + lo;
    }
}

__global__ void __launch_bounds__(1024) k_icp_step(const double *__restrict__ partial, int nblocks, IcpState *__restrict__ st, int64_t ns,
                                                   int mode, int max_it, double rel_fit, double rel_rmse, IcpState *__restrict__ mirror,
                                                   int publish /* this step is one the host waits for (the last step always is) */,
                                                   IcpOrigin org /* origin of the point-to-point slots */) {
    __shared__ double sums[32];
    if (st->done) return;
    // the state the one deciding thread needs, requested BEFORE the reduction so that its round trips run under the partial sums'
    // (they were a chain of dependent loads after the barrier)
    int k = 0;
    double fit0 = 0, rmse0 = 0, T[16];
#pragma unroll
    for (int i = 0; i < 16; i++) T[i] = 0;
    if (threadIdx.x == 0) {
        k = st->evals; fit0 = st->fit; rmse0 = st->rmse;
#pragma unroll
        for (int i = 0; i < 16; i++) T[i] = st->T[i];
    }
    icp_reduce_partials(partial, nblocks, sums);
    __syncthreads();
    if (threadIdx.x != 0) return;
    const unsigned long long now = wall_clock64();
    if (k == 0) st->t_first = now;
    st->t_last = now;
    const double fit = sums[0] / (double)ns, rmse = sums[0] > 0 ? sqrt(sums[1] / sums[0]) : 0.0;
    int stop = 0;
    if (k >= 1 && fabs(fit0 - fit) < rel_fit && fabs(rmse0 - rmse) < rel_rmse) { st->converged = 1; st->iterations = k; stop = 1; }
    else if (k >= max_it) { st->iterations = max_it; stop = 1; }
    st->fit = fit; st->rmse = rmse; st->corr = sums[0];
    st->evals = k + 1;
    if (stop) { st->done = 1; icp_publish(st, mirror); return; }
    double U[16];
    for (int i = 0; i < 16; i++) U[i] = (i % 5 == 0);
    if (sums[0] > 0) {
        if (mode == MODE_P2P) icp_p2p_update(sums, org, U);
        else solve6_to_matrix(sums, U);
    }
    mat4_mul(U, T, T);
    for (int i = 0; i < 16; i++) st->T[i] = T[i];
    if (publish) icp_publish(st, mirror);   // (a publish is ~20 posted writes to host memory and a system-scope fence: not once per step)
}

int upload(r3d_ctx *ctx, DevArena &ar, const double *h, int64_t n3, double **d) {
    return r3d_upload(ctx, ar, h, (size_t)n3, (const double **)d);   // the cores take some of these arrays as non-const rows
}
// the (source, target) pair of a registration problem: ns / nt rows of `width` doubles (3: points, FPFH_DIM: features)
int upload_pair(r3d_ctx *ctx, DevArena &ar, const double *src, int64_t ns, const double *tgt, int64_t nt, double **d_s, double **d_t, int width = 3) {
    if (int rc = upload(ctx, ar, src, ns * width, d_s)) return rc;
    return upload(ctx, ar, tgt, nt * width, d_t);
}
// ... and the M index pairs (source row, target row) of a correspondence problem; M may be 0
int upload_corres_problem(r3d_ctx *ctx, DevArena &ar, const double *src, int64_t ns, const double *tgt, int64_t nt, const int32_t *corres, int64_t M,
                          double **d_s, double **d_t, int **d_c) {
    if (int rc = upload_pair(ctx, ar, src, ns, tgt, nt, d_s, d_t)) return rc;
    return r3d_upload(ctx, ar, corres, (size_t)M * 2, (const int32_t **)d_c);
}
// source.transform(T) of a registered cloud into fresh arena buffers: the points moved, the normals (d_n may be null, *d_on then is) rotated
int transform_cloud(r3d_ctx *ctx, DevArena &ar, const double T[16], const double *d_p, const double *d_n, int64_t n, double **d_o, double **d_on) {
    *d_o = (double *)ar.get((size_t)n * 24);
    *d_on = d_n ? (double *)ar.get((size_t)n * 24) : nullptr;
    if (ar.rc) return ar.rc;
    const unsigned nb = (unsigned)((n + 255) / 256);
    k_transform<<<nb, 256, 0, ctx->stream>>>(d_p, n, to_rigid(T), 0, *d_o);
    if (d_n) k_transform<<<nb, 256, 0, ctx->stream>>>(d_n, n, to_rigid(T), 1, *d_on);
    R3D_HIP(ctx, hipGetLastError());
    return R3D_OK;
}

// ------------------------------------------------------------------------------------------------ RANSAC over correspondences
// The contract is stated in DESIGN.md section 4 ("RANSAC") [recalled, Open3D 0.18 Registration.cpp / CorrespondenceChecker.cpp]
// and executed in tests/ransac_ref.py: a counter-based sampler, the edge-length checker before the transform, Eigen::umeyama
// through umeyama_from_sums, the distance checker, a score over all M pairs whose summation order depends on M alone, and the
// best / stop rule applied in hypothesis order on the host.
constexpr int RANSAC_TILE = 256;            // pairs per LDS tile of k_ransac_score (12 KB)
constexpr int RANSAC_RUN = 1024;            // pairs per summation run: err2 is summed inside a run, the runs are folded in ascending order
constexpr int RANSAC_BLOCK = 256;
constexpr double RANSAC_RANK_TOL = 1e-6;     // umeyama_from_sums' rank test for 3-4 pair samples (see there); the tests' ill-conditioned line
constexpr int RANSAC_MAX_BATCH = 262144, RANSAC_DEFAULT_BATCH = 65536;
constexpr int RANSAC_PIN_SURV = 2048;       // survivors whose results fit the pinned read-back; beyond: a plain copy
constexpr size_t RANSAC_PART_ELEMS = (size_t)16 << 20;   // per-run partials kept at most (runs x survivors); beyond: one share

struct RansacDev {
    unsigned long long seed;
    long long h0;
    int count, n;
    double sim, cd2, max2;                  // edge-length similarity (<= 0: off), checker distance squared (<= 0: off), inlier distance squared
};
struct RansacT { double m[12]; };

__host__ __device__ inline int ransac_sample(unsigned long long seed, long long h, int j, long long M) {
    unsigned long long x = seed + 0x9E3779B97F4A7C15ull * (unsigned long long)(8 * h + j + 1);
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27; x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return (int)(((x >> 32) * (unsigned long long)M) >> 32);
}

// |T s - t|^2 with fused multiply-adds, the one form every stage uses (the distance checker, the score and the winner's mask see
// the same bits).  Inlier and checker tests compare this against the squared threshold: it differs from comparing the rooted
// distance only within a few ulps of the threshold, far inside the 1e-8 band the tests treat as sensitive.
__device__ __forceinline__ double ransac_d2(const double *__restrict__ T, double sx, double sy, double sz, double tx, double ty, double tz) {
    const double dx = fma(T[0], sx, fma(T[1], sy, fma(T[2], sz, T[3]))) - tx;
    const double dy = fma(T[4], sx, fma(T[5], sy, fma(T[6], sz, T[7]))) - ty;
    const double dz = fma(T[8], sx, fma(T[9], sy, fma(T[10], sz, T[11]))) - tz;
    return fma(dz, dz, fma(dy, dy, dx * dx));
}

// pairs[i] = (s, t) of correspondence i, so nothing downstream chases indices; an index outside its cloud is not followed: it
// raises *bad and the row is zeros
__global__ void __launch_bounds__(256) k_ransac_gather(const double *__restrict__ src, int64_t ns, const double *__restrict__ tgt, int64_t nt,
                                                       const int *__restrict__ corres, int64_t M, double *__restrict__ pairs, int *__restrict__ bad) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= M) return;
    const int a = corres[i * 2], b = corres[i * 2 + 1];
    const bool ok = a >= 0 && a < ns && b >= 0 && b < nt;
    if (!ok) *bad = 1;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        pairs[i * 6 + c] = ok ? src[(int64_t)a * 3 + c] : 0.0;
        pairs[i * 6 + 3 + c] = ok ? tgt[(int64_t)b * 3 + c] : 0.0;
    }
}

// k_ransac_propose: one thread per hypothesis of the batch: sample, edge-length checker (a failing thread leaves here), the
// Umeyama sums over the 3-4 pairs, the solve, the distance checker.  Every local array is indexed with constants after
// unrolling (a dynamically indexed one would live in scratch, see umeyama_from_sums).  T is [12][cap]: entry e of slot i at
// T[e * cap + i], coalesced here and in k_ransac_score.  flags: bit 0 edge ok, bit 1 distance ok; valid = both.
__global__ void __launch_bounds__(RANSAC_BLOCK) k_ransac_propose(const double *__restrict__ pairs, int64_t M, RansacDev p, int cap,
                                                                 int *__restrict__ samples /* [count][4] or null */, int *__restrict__ flags,
                                                                 int *__restrict__ valid /* [count + 1] */, double *__restrict__ T) {
    const int i = blockIdx.x * RANSAC_BLOCK + threadIdx.x;
    if (i == 0) valid[p.count] = 0;         // the scan runs over count + 1 entries: its last output is the number of survivors
    if (i >= p.count) return;
    const long long h = p.h0 + i;
    int c[4];
    double P[4][6];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        c[j] = j < p.n ? ransac_sample(p.seed, h, j, M) : -1;
        const int64_t row = c[j < p.n ? j : 0];
#pragma unroll
        for (int q = 0; q < 6; q++) P[j][q] = pairs[row * 6 + q];
    }
    if (samples) {
#pragma unroll
        for (int j = 0; j < 4; j++) samples[(int64_t)i * 4 + j] = c[j];
    }
    bool edge = true;
    if (p.sim > 0.0) {
#pragma unroll
        for (int a = 0; a < 4; a++)
#pragma unroll
            for (int b = a + 1; b < 4; b++) {
                if (b >= p.n) continue;
                const double sx = P[a][0] - P[b][0], sy = P[a][1] - P[b][1], sz = P[a][2] - P[b][2];
                const double tx = P[a][3] - P[b][3], ty = P[a][4] - P[b][4], tz = P[a][5] - P[b][5];
                const double ds = sqrt((sx * sx + sy * sy) + sz * sz), dt = sqrt((tx * tx + ty * ty) + tz * tz);
                if (!(ds >= p.sim * dt && dt >= p.sim * ds)) edge = false;
            }
    }
    if (!edge) { flags[i] = 0; valid[i] = 0; return; }
    double s[17];
#pragma unroll
    for (int q = 0; q < 17; q++) s[q] = 0.0;
    s[0] = (double)p.n;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        if (j >= p.n) continue;
#pragma unroll
        for (int a = 0; a < 3; a++) {
            s[2 + a] += P[j][a];
            s[5 + a] += P[j][3 + a];
#pragma unroll
            for (int b = 0; b < 3; b++) s[8 + a * 3 + b] += P[j][a] * P[j][3 + b];
        }
    }
    double U[16];
    umeyama_from_sums(s, U, RANSAC_RANK_TOL);
    umeyama_polish(s, U);
    bool dist = true;
    if (p.cd2 > 0.0) {
#pragma unroll
        for (int j = 0; j < 4; j++)
            if (j < p.n && ransac_d2(U, P[j][0], P[j][1], P[j][2], P[j][3], P[j][4], P[j][5]) > p.cd2) dist = false;
    }
#pragma unroll
    for (int e = 0; e < 12; e++) T[(int64_t)e * cap + i] = U[e];
    flags[i] = dist ? 3 : 1;
    valid[i] = dist ? 1 : 0;
}

// survivors in h order: surv[rank] = batch slot (the ranks come from the exclusive scan of valid)
__global__ void __launch_bounds__(256) k_ransac_compact(const int *__restrict__ valid, const int *__restrict__ scan, int count, int *__restrict__ surv) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < count && valid[i]) surv[scan[i]] = i;
}

// k_ransac_score: one surviving hypothesis per thread, its 12 transform entries in registers; the pairs of this block's share
// (blockIdx.y of gridDim.y equal groups of runs) are staged RANSAC_TILE at a time in LDS and read by every lane at one address
// (a broadcast, the shape of k_match_features).  Inside a run the count and the squared distances of the inliers are summed in
// pair order.  DIRECT (one share): the thread folds its runs in ascending order itself and writes the result; otherwise it
// leaves (count, err2) per run in part_*[run * nsurv + k] and k_ransac_reduce folds them in the same order, so both give the
// same bits whatever the grid.
template <bool DIRECT>
__global__ void __launch_bounds__(RANSAC_BLOCK) k_ransac_score(const double *__restrict__ pairs, int64_t M, const double *__restrict__ T, int cap,
                                                               const int *__restrict__ surv, int nsurv, int runs_per_share, int nruns, double max2,
                                                               int *__restrict__ out_cnt, double *__restrict__ out_err) {
    __shared__ double tile[RANSAC_TILE * 6];
    const int k = blockIdx.x * RANSAC_BLOCK + threadIdx.x;
    const int slot = surv[k < nsurv ? k : nsurv - 1];   // a lane past the end works on the last survivor (it takes part in the staging) and writes nothing
    double t[12];
#pragma unroll
    for (int e = 0; e < 12; e++) t[e] = T[(int64_t)e * cap + slot];
    const int r0 = blockIdx.y * runs_per_share, r1 = min(nruns, r0 + runs_per_share);
    int tot_c = 0;
    double tot_e = 0.0;
    for (int run = r0; run < r1; run++) {
        const int64_t b0 = (int64_t)run * RANSAC_RUN, b1 = b0 + RANSAC_RUN < M ? b0 + RANSAC_RUN : M;
        int cnt = 0;
        double err = 0.0;
        for (int64_t tb = b0; tb < b1; tb += RANSAC_TILE) {
            const int rows = (int)(b1 - tb < RANSAC_TILE ? b1 - tb : RANSAC_TILE);
            __syncthreads();
            for (int e = threadIdx.x; e < rows * 6; e += RANSAC_BLOCK) tile[e] = pairs[tb * 6 + e];
            __syncthreads();
#pragma unroll 4
            for (int r = 0; r < rows; r++) {
                const double *__restrict__ q = tile + r * 6;
                const double d2 = ransac_d2(t, q[0], q[1], q[2], q[3], q[4], q[5]);
                const bool in = d2 < max2;
                cnt += in ? 1 : 0;
                err += in ? d2 : 0.0;       // adding +0 leaves the sum as it is: no branch, same bits
            }
        }
        if (DIRECT) { tot_c += cnt; tot_e += err; }
        else if (k < nsurv) { out_cnt[(int64_t)run * nsurv + k] = cnt; out_err[(int64_t)run * nsurv + k] = err; }
    }
    if (DIRECT && k < nsurv) { out_cnt[k] = tot_c; out_err[k] = tot_e; }
}
__global__ void __launch_bounds__(256) k_ransac_reduce(const int *__restrict__ part_cnt, const double *__restrict__ part_err, int nsurv, int nruns,
                                                       int *__restrict__ cnt, double *__restrict__ err) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= nsurv) return;
    int c = 0;
    double e = 0.0;
    for (int run = 0; run < nruns; run++) { c += part_cnt[(int64_t)run * nsurv + k]; e += part_err[(int64_t)run * nsurv + k]; }
    cnt[k] = c;
    err[k] = e;
}
// the transform of one batch slot as 12 consecutive doubles (the host's read-back of a new best)
__global__ void __launch_bounds__(64) k_ransac_fetch_T(const double *__restrict__ T, int cap, int slot, double *__restrict__ out12) {
    if (threadIdx.x < 12) out12[threadIdx.x] = T[(int64_t)threadIdx.x * cap + slot];
}
// the winner's inlier mask, with the arithmetic of the score
__global__ void __launch_bounds__(256) k_ransac_mask(const double *__restrict__ pairs, int64_t M, RansacT T, double max2, unsigned char *__restrict__ mask) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= M) return;
    const double *__restrict__ q = pairs + i * 6;
    mask[i] = ransac_d2(T.m, q[0], q[1], q[2], q[3], q[4], q[5]) < max2 ? 1 : 0;
}

// ---- RANSAC over correspondences: the host side
struct RansacWork {
    double *pairs = nullptr, *T = nullptr, *res_err = nullptr, *part_err = nullptr, *T12 = nullptr;
    int *samples = nullptr, *flags = nullptr, *valid = nullptr, *scan = nullptr, *surv = nullptr, *res_cnt = nullptr, *part_cnt = nullptr, *bad = nullptr,
        *scan_part = nullptr;               // the scan's tile sums, taken once: every batch scans on the same stream
    int cap = 0, nruns = 0;
    size_t part_elems = 0;
};

// the pairs gathered and their indices checked (one read-back, before any hypothesis reads a pair), the batch buffers reserved
int ransac_setup(r3d_ctx *ctx, DevArena &ar, const double *d_src, int64_t ns, const double *d_tgt, int64_t nt, const int *d_corres, int64_t M,
                 int cap, bool want_samples, RansacWork &W) {
    W.cap = cap;
    W.nruns = (int)((M + RANSAC_RUN - 1) / RANSAC_RUN);
    size_t part_cap = RANSAC_PART_ELEMS;
    if (const char *e = getenv("R3D_RANSAC_PART_ELEMS")) part_cap = (size_t)std::max<long long>(atoll(e), 0);   // diagnostic: 0 forces the one-share path
    W.part_elems = std::min<size_t>((size_t)W.nruns * cap, part_cap);
    W.pairs = (double *)ar.get((size_t)M * 48);
    W.T = (double *)ar.get((size_t)cap * 96);
    W.res_err = (double *)ar.get((size_t)cap * 8);
    W.part_err = (double *)ar.get(W.part_elems * 8);
    W.T12 = (double *)ar.get(96);
    W.samples = want_samples ? (int *)ar.get((size_t)cap * 16) : nullptr;
    W.flags = (int *)ar.get((size_t)cap * 4);
    W.valid = (int *)ar.get((size_t)(cap + 1) * 4);
    W.scan = (int *)ar.get((size_t)(cap + 1) * 4);
    W.surv = (int *)ar.get((size_t)cap * 4);
    W.res_cnt = (int *)ar.get((size_t)cap * 4);
    W.part_cnt = (int *)ar.get(W.part_elems * 4);
    W.bad = (int *)ar.get(4);
    W.scan_part = (int *)ar.get((size_t)((cap + 1 + SCAN_TILE - 1) / SCAN_TILE) * 4);
    if (ar.rc) return ar.rc;
    R3D_HIP(ctx, hipMemsetAsync(W.bad, 0, 4, ctx->stream));
    k_ransac_gather<<<(unsigned)((M + 255) / 256), 256, 0, ctx->stream>>>(d_src, ns, d_tgt, nt, d_corres, M, W.pairs, W.bad);
    R3D_HIP(ctx, hipGetLastError());
    int bad = 0;
    PinRead rd(ctx);
    int rc;
    if ((rc = rd.add(&bad, W.bad, 4)) || (rc = rd.wait())) return rc;
    if (bad) return r3d_fail(ctx, R3D_E_BADARG, "ransac: a correspondence index lies outside its cloud (ns = %lld, nt = %lld)", (long long)ns, (long long)nt);
    return R3D_OK;
}

// hypotheses pd.h0 .. pd.h0 + pd.count - 1: proposed, compacted in h order and scored; leaves surv / res_cnt / res_err [nsurv]
int ransac_batch(r3d_ctx *ctx, DevArena &ar, const RansacWork &W, int64_t M, const RansacDev &pd, int *nsurv_out) {
    const int count = pd.count;
    k_ransac_propose<<<(unsigned)((count + RANSAC_BLOCK - 1) / RANSAC_BLOCK), RANSAC_BLOCK, 0, ctx->stream>>>(W.pairs, M, pd, W.cap, W.samples, W.flags,
                                                                                                             W.valid, W.T);
    R3D_HIP(ctx, hipGetLastError());
    int rc;
    if ((rc = dev_exclusive_scan<int>(ctx, ar, W.valid, W.scan, (int64_t)count + 1, nullptr, nullptr, W.scan_part))) return rc;
    k_ransac_compact<<<(unsigned)((count + 255) / 256), 256, 0, ctx->stream>>>(W.valid, W.scan, count, W.surv);
    R3D_HIP(ctx, hipGetLastError());
    int nsurv = 0;
    {
        PinRead rd(ctx);
        if ((rc = rd.add(&nsurv, W.scan + count, 4)) || (rc = rd.wait())) return rc;
    }
    *nsurv_out = nsurv;
    if (nsurv <= 0) return R3D_OK;
    // few survivors: the runs are split over gridDim.y so that the chip is still filled (about 2048 workgroups)
    const int nbx = (nsurv + RANSAC_BLOCK - 1) / RANSAC_BLOCK;
    int shares = std::max(1, std::min(W.nruns, 2048 / nbx));
    if ((size_t)W.nruns * nsurv > W.part_elems) shares = 1;
    const int per = (W.nruns + shares - 1) / shares;
    shares = (W.nruns + per - 1) / per;
    if (shares == 1) {
        k_ransac_score<true><<<dim3(nbx, 1), RANSAC_BLOCK, 0, ctx->stream>>>(W.pairs, M, W.T, W.cap, W.surv, nsurv, W.nruns, W.nruns, pd.max2, W.res_cnt,
                                                                          W.res_err);
    } else {
        k_ransac_score<false><<<dim3(nbx, shares), RANSAC_BLOCK, 0, ctx->stream>>>(W.pairs, M, W.T, W.cap, W.surv, nsurv, per, W.nruns, pd.max2,
                                                                                W.part_cnt, W.part_err);
        k_ransac_reduce<<<(unsigned)((nsurv + 255) / 256), 256, 0, ctx->stream>>>(W.part_cnt, W.part_err, nsurv, W.nruns, W.res_cnt, W.res_err);
    }
    R3D_HIP(ctx, hipGetLastError());
    return R3D_OK;
}

// surv / res_cnt / res_err of the last batch on the host: through the pinned buffer when they fit, a plain copy otherwise
int ransac_read_results(r3d_ctx *ctx, const RansacWork &W, int nsurv, std::vector<int> &surv, std::vector<int> &cnt, std::vector<double> &err) {
    surv.resize(nsurv); cnt.resize(nsurv); err.resize(nsurv);
    if (nsurv <= RANSAC_PIN_SURV) {
        PinRead rd(ctx);
        int rc;
        if ((rc = rd.add(surv.data(), W.surv, (size_t)nsurv * 4)) || (rc = rd.add(cnt.data(), W.res_cnt, (size_t)nsurv * 4)) ||
            (rc = rd.add(err.data(), W.res_err, (size_t)nsurv * 8)) || (rc = rd.wait()))
            return rc;
        return R3D_OK;
    }
    R3D_HIP(ctx, hipMemcpyAsync(surv.data(), W.surv, (size_t)nsurv * 4, hipMemcpyDeviceToHost, ctx->stream));
    R3D_HIP(ctx, hipMemcpyAsync(cnt.data(), W.res_cnt, (size_t)nsurv * 4, hipMemcpyDeviceToHost, ctx->stream));
    R3D_HIP(ctx, hipMemcpyAsync(err.data(), W.res_err, (size_t)nsurv * 8, hipMemcpyDeviceToHost, ctx->stream));
    R3D_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return R3D_OK;
}

RansacDev ransac_dev_params(const r3d_ransac_params *p) {
    RansacDev pd;
    pd.seed = p->seed;
    pd.h0 = 0;
    pd.count = 0;
    pd.n = p->ransac_n;
    pd.sim = p->edge_length_similarity > 0 ? p->edge_length_similarity : 0.0;
    pd.cd2 = p->checker_distance > 0 ? p->checker_distance * p->checker_distance : 0.0;
    pd.max2 = p->max_correspondence_distance * p->max_correspondence_distance;
    return pd;
}

int ransac_check(r3d_ctx *ctx, const char *who, const r3d_ransac_params *p, const void *src, int64_t ns, const void *tgt, int64_t nt, const void *corres,
                 int64_t M) {
    if (!p || !src || !tgt || !corres || ns <= 0 || nt <= 0) return r3d_fail(ctx, R3D_E_BADARG, "%s: bad argument (null array or empty cloud)", who);
    if (p->ransac_n < 3 || p->ransac_n > 4) return r3d_fail(ctx, R3D_E_UNSUPPORTED, "%s: ransac_n = %d not supported (3 or 4)", who, p->ransac_n);
    if (M < p->ransac_n) return r3d_fail(ctx, R3D_E_BADARG, "%s: %lld correspondences, fewer than ransac_n = %d", who, (long long)M, p->ransac_n);
    if (!(p->max_correspondence_distance > 0) || !(p->confidence > 0) || p->max_iteration < 1)
        return r3d_fail(ctx, R3D_E_BADARG, "%s: max_correspondence_distance and confidence must be > 0, max_iteration >= 1", who);
    if (p->max_iteration > 0x7fffffff || M > 0x7fffffff || ns > 0x7fffffff || nt > 0x7fffffff)
        return r3d_fail(ctx, R3D_E_UNSUPPORTED, "%s: max_iteration, M, ns and nt must stay below 2^31", who);
    return R3D_OK;
}

// rule 6 of the contract: how many hypotheses a best of this fitness still asks for (host double arithmetic with libm, which the
// restatement repeats through Python's math module)
int64_t ransac_est_k(double fitness, int n, double confidence, int64_t max_iteration) {
    if (confidence >= 1.0) return max_iteration;
    const double pw = std::pow(fitness, (double)n);
    if (pw >= 1.0) return 0;
    if (!(pw > 0.0)) return max_iteration;
    const double k = std::ceil(std::log(1.0 - confidence) / std::log1p(-pw));
    return k < (double)max_iteration ? (int64_t)k : max_iteration;
}

// the loop over device arrays.  mask_dev / mask_host: where the winner's mask goes (either may be null).
int ransac_core(r3d_ctx *ctx, DevArena &ar, const r3d_ransac_params *p, const double *d_src, int64_t ns, const double *d_tgt, int64_t nt,
                const int *d_corres, int64_t M, double *T4x4, unsigned char *mask_dev, unsigned char *mask_host, r3d_ransac_stats *stats,
                std::chrono::steady_clock::time_point t_begin) {
    const int64_t max_it = p->max_iteration;
    const int batch = (int)std::min<int64_t>(std::max<int64_t>(p->batch > 0 ? p->batch : RANSAC_DEFAULT_BATCH, 1), std::min<int64_t>(RANSAC_MAX_BATCH, max_it));
    RansacWork W;
    int rc;
    if ((rc = ransac_setup(ctx, ar, d_src, ns, d_tgt, nt, d_corres, M, batch, false, W))) return rc;
    unsigned char *d_mask = mask_dev ? mask_dev : (mask_host ? (unsigned char *)ar.get((size_t)M) : nullptr);
    if (ar.rc) return ar.rc;
    const auto t_loop = std::chrono::steady_clock::now();
    RansacDev pd = ransac_dev_params(p);
    int64_t limit = max_it, h0 = 0, validated = 0, best_h = -1, best_cnt = 0;
    double best_rmse = 0.0, bestT[12];
    std::vector<int> surv, cnt;
    std::vector<double> err;
    while (h0 < limit) {
        pd.h0 = h0;
        pd.count = (int)std::min<int64_t>(batch, limit - h0);
        int nsurv = 0;
        if ((rc = ransac_batch(ctx, ar, W, M, pd, &nsurv))) return rc;
        if (nsurv > 0) {
            if ((rc = ransac_read_results(ctx, W, nsurv, surv, cnt, err))) return rc;
            int new_best_slot = -1;
            for (int k = 0; k < nsurv; k++) {
                const int64_t h = h0 + surv[k];
                if (h >= limit) break;      // the sequential walk has stopped: the rest of the batch was wasted work
                validated++;
                if (cnt[k] <= 0) continue;
                const double rmse = std::sqrt(err[k] / (double)cnt[k]);
                if (cnt[k] > best_cnt || (cnt[k] == best_cnt && rmse < best_rmse)) {
                    best_cnt = cnt[k]; best_rmse = rmse; best_h = h; new_best_slot = surv[k];
                    const int64_t est = ransac_est_k((double)cnt[k] / (double)M, p->ransac_n, p->confidence, max_it);
                    limit = std::max<int64_t>(std::min<int64_t>(max_it, est), h + 1);
                }
            }
            if (new_best_slot >= 0) {       // the arena's T is overwritten by the next batch
                k_ransac_fetch_T<<<1, 64, 0, ctx->stream>>>(W.T, W.cap, new_best_slot, W.T12);
                R3D_HIP(ctx, hipGetLastError());
                PinRead rd(ctx);
                if ((rc = rd.add(bestT, W.T12, 96)) || (rc = rd.wait())) return rc;
            }
        }
        h0 += pd.count;
    }
    for (int i = 0; i < 16; i++) T4x4[i] = (i % 5 == 0);
    if (best_h >= 0) memcpy(T4x4, bestT, 96);
    if (d_mask) {
        if (best_h >= 0) {
            RansacT Tm;
            memcpy(Tm.m, bestT, 96);
            k_ransac_mask<<<(unsigned)((M + 255) / 256), 256, 0, ctx->stream>>>(W.pairs, M, Tm, pd.max2, d_mask);
            R3D_HIP(ctx, hipGetLastError());
        } else {
            R3D_HIP(ctx, hipMemsetAsync(d_mask, 0, (size_t)M, ctx->stream));
        }
        if ((rc = r3d_download(ctx, mask_host, d_mask, (size_t)M))) return rc;
    }
    R3D_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (stats) {
        stats->fitness = best_h >= 0 ? (double)best_cnt / (double)M : 0.0;
        stats->inlier_rmse = best_h >= 0 ? best_rmse : 0.0;
        stats->iterations = limit;
        stats->validated = validated;
        stats->best_hypothesis = best_h;
        stats->inliers = best_cnt;
        const auto t_end = std::chrono::steady_clock::now();
        stats->setup_ms = std::chrono::duration<double, std::milli>(t_loop - t_begin).count();
        stats->loop_ms = std::chrono::duration<double, std::milli>(t_end - t_loop).count();
    }
    return R3D_OK;
}

// ------------------------------------------------------------------------------------------------ Fast Global Registration
// The contract is stated in DESIGN.md section 4 ("FGR") [recalled, Open3D 0.18 FastGlobalRegistration.cpp] and executed in
// tests/fgr_ref.py: both clouds centred and scaled, the pairs (given, or the mutual ones of two feature searches), the tuple test
// with RANSAC's counter-based sampler, the graduated-non-convexity Gauss-Newton loop, the result in the clouds' own units.
// Every sum below has one fixed order that depends on the sizes alone: the same bits on every run, whatever `batch` is.
constexpr int FGR_MIN_PAIRS = 10;           // fewer rows: the loop does not run (Open3D's OptimizePairwiseRegistration)
constexpr int FGR_TRIALS_PER_PAIR = 100;
constexpr int FGR_OPT_BLOCK = 1024, FGR_OPT_WAVES = FGR_OPT_BLOCK / 64;
constexpr int FGR_SUMS = 16;                // the distinct ones of the 21 + 6 sums, see k_fgr_optimize
constexpr int FGR_MOM_BLOCKS = 1024;

struct FgrNorm { double mean_s[3], mean_t[3], scale_global; };

// sums of the coordinates of both clouds (blockIdx.y: 0 source, 1 target): thread-strided partial sums, then a fixed tree in LDS;
// part[(y * gridDim.x + b) * 3 + a]
__global__ void __launch_bounds__(256) k_fgr_moments(const double *__restrict__ src, int64_t ns, const double *__restrict__ tgt, int64_t nt,
                                                     double *__restrict__ part) {
    const double *__restrict__ p = blockIdx.y ? tgt : src;
    const int64_t n = blockIdx.y ? nt : ns;
    double s[3] = {0.0, 0.0, 0.0};
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
        for (int a = 0; a < 3; a++) s[a] += p[i * 3 + a];
    __shared__ double sm[3][256];
    for (int a = 0; a < 3; a++) sm[a][threadIdx.x] = s[a];
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h)
            for (int a = 0; a < 3; a++) sm[a][threadIdx.x] += sm[a][threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x < 3) part[((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * 3 + threadIdx.x] = sm[threadIdx.x][0];
}
// the finish: the partial sums folded the same way, divided by n; mom[0..2] mean_s, mom[3..5] mean_t
__global__ void __launch_bounds__(256) k_fgr_moments_final(const double *__restrict__ part, int nb, int64_t ns, int64_t nt, double *__restrict__ mom) {
    __shared__ double sm[6][256];
    for (int c = 0; c < 2; c++) {
        double s[3] = {0.0, 0.0, 0.0};
        for (int b = threadIdx.x; b < nb; b += 256)
            for (int a = 0; a < 3; a++) s[a] += part[((int64_t)c * nb + b) * 3 + a];
        for (int a = 0; a < 3; a++) sm[c * 3 + a][threadIdx.x] = s[a];
    }
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h)
            for (int a = 0; a < 6; a++) sm[a][threadIdx.x] += sm[a][threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x < 6) mom[threadIdx.x] = sm[threadIdx.x][0] / (double)(threadIdx.x < 3 ? ns : nt);
}
// the largest norm of the centred points, per workgroup (a maximum: any order gives the same value)
__global__ void __launch_bounds__(256) k_fgr_maxnorm(const double *__restrict__ src, int64_t ns, const double *__restrict__ tgt, int64_t nt,
                                                     const double *__restrict__ mom, double *__restrict__ part) {
    const double *__restrict__ p = blockIdx.y ? tgt : src;
    const int64_t n = blockIdx.y ? nt : ns;
    const double mx = mom[blockIdx.y * 3], my = mom[blockIdx.y * 3 + 1], mz = mom[blockIdx.y * 3 + 2];
    double m = 0.0;
    bool bad = false;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const double x = p[i * 3] - mx, y = p[i * 3 + 1] - my, z = p[i * 3 + 2] - mz;
        const double l = sqrt((x * x + y * y) + z * z);
        bad |= !isfinite(l);                // fmax drops a NaN: it is carried separately
        m = fmax(m, l);
    }
    __shared__ double sm[256];
    sm[threadIdx.x] = bad ? INFINITY : m;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) sm[threadIdx.x] = fmax(sm[threadIdx.x], sm[threadIdx.x + h]);
        __syncthreads();
    }
    if (threadIdx.x == 0) part[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = sm[0];
}
__global__ void __launch_bounds__(256) k_fgr_maxnorm_final(const double *__restrict__ part, int nb2, double *__restrict__ mom) {
    __shared__ double sm[256];
    double m = 0.0;
    for (int b = threadIdx.x; b < nb2; b += 256) m = fmax(m, part[b]);
    sm[threadIdx.x] = m;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) sm[threadIdx.x] = fmax(sm[threadIdx.x], sm[threadIdx.x + h]);
        __syncthreads();
    }
    if (threadIdx.x == 0) { mom[6] = sm[0]; mom[7] = 0.0; }
}

// the plain cross-check of the two feature searches: flag[i] = nn_ts[nn_st[i]] == i (flag[ns] = 0: the scan's last output is the
// count); an index outside its table is not followed
__global__ void __launch_bounds__(256) k_fgr_mutual(const int *__restrict__ nn_st, int64_t ns, const int *__restrict__ nn_ts, int64_t nt,
                                                    int *__restrict__ flag) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i > ns) return;
    int f = 0;
    if (i < ns) {
        const int j = nn_st[i];
        if (j >= 0 && j < nt) f = nn_ts[j] == (int)i ? 1 : 0;
    }
    flag[i] = f;
}
// the mutual pairs in ascending i
__global__ void __launch_bounds__(256) k_fgr_mutual_compact(const int *__restrict__ nn_st, int64_t ns, const int *__restrict__ flag,
                                                            const int *__restrict__ scan, int *__restrict__ corres) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= ns || !flag[i]) return;
    corres[(int64_t)scan[i] * 2] = (int)i;
    corres[(int64_t)scan[i] * 2 + 1] = nn_st[i];
}

// rows[i] = (p, q) of pair i, centred and divided by scale_global; an index outside its cloud is not followed: it raises *bad
// and the row is zeros
__global__ void __launch_bounds__(256) k_fgr_gather(const double *__restrict__ src, int64_t ns, const double *__restrict__ tgt, int64_t nt,
                                                    const int *__restrict__ corres, int64_t M, FgrNorm nm, double *__restrict__ rows,
                                                    int *__restrict__ bad) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= M) return;
    const int a = corres[i * 2], b = corres[i * 2 + 1];
    const bool ok = a >= 0 && a < ns && b >= 0 && b < nt;
    if (!ok) *bad = 1;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        rows[i * 6 + c] = ok ? (src[(int64_t)a * 3 + c] - nm.mean_s[c]) / nm.scale_global : 0.0;
        rows[i * 6 + 3 + c] = ok ? (tgt[(int64_t)b * 3 + c] - nm.mean_t[c]) / nm.scale_global : 0.0;
    }
}

// one trial of the tuple test per thread: the three pair indices from RANSAC's sampler (no distinctness test: a repeated index
// gives a zero edge, and 0 < 0 fails), then li * tuple_scale < lj < li / tuple_scale on the three edges.  flags[count] = 0: the
// scan's last output is the number of accepted trials of the batch.
__global__ void __launch_bounds__(256) k_fgr_tuples(const double *__restrict__ rows, int64_t ncorr, unsigned long long seed, long long t0, int count,
                                                    double tuple_scale, int *__restrict__ samples /* [count][3] or null */,
                                                    int *__restrict__ flags /* [count + 1] */, int *__restrict__ cut /* or null: set to -1 */) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i == 0) { flags[count] = 0; if (cut) *cut = -1; }
    if (i >= count) return;
    int c[3];
    double P[3][6];
#pragma unroll
    for (int j = 0; j < 3; j++) {
        c[j] = ransac_sample(seed, t0 + i, j, ncorr);
#pragma unroll
        for (int q = 0; q < 6; q++) P[j][q] = rows[(int64_t)c[j] * 6 + q];
    }
    if (samples) {
#pragma unroll
        for (int j = 0; j < 3; j++) samples[(int64_t)i * 3 + j] = c[j];
    }
    bool ok = true;
#pragma unroll
    for (int e = 0; e < 3; e++) {
        const int a = e, b = (e + 1) % 3;   // (r0, r1), (r1, r2), (r2, r0)
        const double sx = P[a][0] - P[b][0], sy = P[a][1] - P[b][1], sz = P[a][2] - P[b][2];
        const double tx = P[a][3] - P[b][3], ty = P[a][4] - P[b][4], tz = P[a][5] - P[b][5];
        const double li = sqrt((sx * sx + sy * sy) + sz * sz), lj = sqrt((tx * tx + ty * ty) + tz * tz);
        if (!(li * tuple_scale < lj && lj < li / tuple_scale)) ok = false;
    }
    flags[i] = ok ? 1 : 0;
}
// the accepted trials of a batch in t order behind the `have` accepted before it, the cut at `max_count`: trial rank r < max_count
// leaves its three rows at out[3 r ..]; the one that fills the last place leaves its batch slot in *cut (set to -1 before)
__global__ void __launch_bounds__(256) k_fgr_tuple_compact(const double *__restrict__ rows, int64_t ncorr, unsigned long long seed, long long t0,
                                                           int count, const int *__restrict__ flags, const int *__restrict__ scan, int64_t have,
                                                           int64_t max_count, double *__restrict__ out, int *__restrict__ cut) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= count || !flags[i]) return;
    const int64_t r = have + scan[i];
    if (r >= max_count) return;
    if (r == max_count - 1) *cut = i;
#pragma unroll
    for (int j = 0; j < 3; j++) {
        const int64_t c = ransac_sample(seed, t0 + i, j, ncorr);
#pragma unroll
        for (int q = 0; q < 6; q++) out[(r * 3 + j) * 6 + q] = rows[c * 6 + q];
    }
}

// k_fgr_optimize: the whole graduated-non-convexity loop in one launch by one workgroup; no launch and no host read between its
// iterations.  Per iteration every thread walks the rows tid, tid + 1024, ... in ascending order: q = trans q0, rpq = p - q,
// s = (par / (rpq . rpq + par))^2, and the sums of s J^T J and s J^T r with the three Jacobian rows [0, -qz, qy, -1, 0, 0],
// [qz, 0, -qx, 0, -1, 0], [-qy, qx, 0, 0, 0, -1].  Of those 21 + 6 sums only 16 differ: six of the rotation block, S s q (the
// rotation-translation block holds it and its exact negative), S s (the translation block's diagonal) and the six right-hand
// sides; the others are sums of exact zeros.  The 16 are reduced per wave by wave_sum's fixed tree and across the 16 waves
// through LDS in wave order; thread 0 then expands them into solve6_to_matrix's slots, solves without the determinant rule,
// forms trans = delta trans and publishes it in LDS for the next iteration.
// out17: the final trans and par; trace_T [iterations][16] / trace_par [iterations] (both or neither): the state after every
// iteration (r3d_debug_fgr_optimize).
__global__ void __launch_bounds__(FGR_OPT_BLOCK) k_fgr_optimize(const double *__restrict__ rows, int64_t M, int iterations, double par0, double limit,
                                                                double division_factor, int decrease_mu, double *__restrict__ out17,
                                                                double *__restrict__ trace_T, double *__restrict__ trace_par) {
    __shared__ double wsum[FGR_OPT_WAVES][FGR_SUMS];
    __shared__ double sh_state[13];         // rows 0..2 of trans, par
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    double T[16], par = par0;               // thread 0's copy is the state
#pragma unroll
    for (int i = 0; i < 16; i++) T[i] = (i % 5 == 0);
    if (tid < 12) sh_state[tid] = (tid % 5 == 0) ? 1.0 : 0.0;
    if (tid == 12) sh_state[12] = par0;
    __syncthreads();
    for (int itr = 0; itr < iterations; itr++) {
        double t[12];
#pragma unroll
        for (int i = 0; i < 12; i++) t[i] = sh_state[i];
        const double pr = sh_state[12];
        double acc[FGR_SUMS];
#pragma unroll
        for (int e = 0; e < FGR_SUMS; e++) acc[e] = 0.0;
#pragma unroll 2
        for (int64_t i = tid; i < M; i += FGR_OPT_BLOCK) {
            const double *__restrict__ r = rows + i * 6;
            const double px = r[0], py = r[1], pz = r[2], x0 = r[3], y0 = r[4], z0 = r[5];
            const double qx = ((t[0] * x0 + t[1] * y0) + t[2] * z0) + t[3];
            const double qy = ((t[4] * x0 + t[5] * y0) + t[6] * z0) + t[7];
            const double qz = ((t[8] * x0 + t[9] * y0) + t[10] * z0) + t[11];
            const double rx = px - qx, ry = py - qy, rz = pz - qz;
            const double wt = pr / (((rx * rx + ry * ry) + rz * rz) + pr);
            const double s = wt * wt;
            acc[0] += s * (qy * qy + qz * qz);
            acc[1] += s * -(qx * qy);
            acc[2] += s * -(qx * qz);
            acc[3] += s * (qx * qx + qz * qz);
            acc[4] += s * -(qy * qz);
            acc[5] += s * (qx * qx + qy * qy);
            acc[6] += s * qx;
            acc[7] += s * qy;
            acc[8] += s * qz;
            acc[9] += s;
            acc[10] += s * (qz * ry - qy * rz);
            acc[11] += s * (qx * rz - qz * rx);
            acc[12] += s * (qy * rx - qx * ry);
            acc[13] += s * -rx;
            acc[14] += s * -ry;
            acc[15] += s * -rz;
        }
#pragma unroll
        for (int e = 0; e < FGR_SUMS; e++) {
            const double v = wave_sum(acc[e]);
            if (lane == 0) wsum[w][e] = v;
        }
        __syncthreads();
        if (tid == 0) {
            double v[FGR_SUMS];
            for (int e = 0; e < FGR_SUMS; e++) {
                double a = 0.0;
                for (int k = 0; k < FGR_OPT_WAVES; k++) a += wsum[k][e];
                v[e] = a;
            }
            // solve6_to_matrix's slots: [2 .. 22] the upper triangle of JTJ row by row, [23 .. 28] JTr
            const double sx = v[6], sy = v[7], sz = v[8], ss = v[9];
            const double sl[29] = {0.0, 0.0,
                                   v[0], v[1], v[2], 0.0, -sz, sy,
                                   v[3], v[4], sz, 0.0, -sx,
                                   v[5], -sy, sx, 0.0,
                                   ss, 0.0, 0.0,
                                   ss, 0.0,
                                   ss,
                                   v[10], v[11], v[12], v[13], v[14], v[15]};
            double U[16];
            solve6_to_matrix(sl, U, -1.0);  // a failed solve leaves the identity: the loop goes on
            mat4_mul(U, T, T);
            if (decrease_mu && itr % 4 == 0 && par > limit) par /= division_factor;
            for (int i = 0; i < 12; i++) sh_state[i] = T[i];
            sh_state[12] = par;
            if (trace_T) {
                for (int i = 0; i < 16; i++) trace_T[(int64_t)itr * 16 + i] = T[i];
                trace_par[itr] = par;
            }
        }
        __syncthreads();
    }
    if (tid == 0) {
        for (int i = 0; i < 16; i++) out17[i] = T[i];
        out17[16] = par;
    }
}

}  // namespace

// the int32 scan for the other translation units (trimesh.hip)
int r3d_exclusive_scan_i32(r3d_ctx *ctx, DevArena &ar, const int *in, int *out, int64_t n) { return dev_exclusive_scan<int>(ctx, ar, in, out, n); }

// the stable by-cell order for poisson.hip: voxel keys (key_order 1: floor((p - org) / cell) per axis with a true division, clamped
// to the grid; key = (cx * dims[1] + cy) * dims[2] + cz), which must fit 32 bits
int r3d_sort_by_voxel_u32(r3d_ctx *ctx, DevArena &ar, const double *d_pts, int64_t n, const double org[3], double cell, const int dims[3],
                          const unsigned **keys_sorted, const int **idx_sorted) {
    void *keys = nullptr;
    int *idx = nullptr;
    bool k32 = false;
    if (int rc = sort_by_cell(ctx, ar, d_pts, n, org, cell, dims, 1, &keys, &k32, &idx)) return rc;
    if (!k32) return r3d_fail(ctx, R3D_E_UNSUPPORTED, "sort_by_voxel_u32: a %d x %d x %d grid needs 64-bit keys", dims[0], dims[1], dims[2]);
    *keys_sorted = (const unsigned *)keys;
    *idx_sorted = idx;
    return R3D_OK;
}

// the radix sort itself for meshtopo.hip: n (key, value) pairs in the stable order of the keys' low `bits` bits (at least one pass,
// eight bits each), values = the index where d_vals is null.  The inputs are only read; the results are arena buffers.  Enqueued on
// the ctx stream, no host round trip.  Positions are int32: n above 2^31 - 1 is refused.
int r3d_sort_pairs_u64(r3d_ctx *ctx, DevArena &ar, const uint64_t *d_keys, const int *d_vals, int64_t n, int bits, const uint64_t **keys_sorted,
                       const int **vals_sorted) {
    *keys_sorted = nullptr;
    *vals_sorted = nullptr;
    if (n < 0 || bits < 0 || bits > 64) return r3d_fail(ctx, R3D_E_BADARG, "sort_pairs_u64: %lld pairs on %d bits", (long long)n, bits);
    if (n > 0x7fffffff) return r3d_fail(ctx, R3D_E_UNSUPPORTED, "sort_pairs_u64: %lld pairs do not fit int32 positions", (long long)n);
    if (n == 0) return R3D_OK;
    using KEY = unsigned long long;
    KEY *k[2] = {(KEY *)ar.get((size_t)n * 8), (KEY *)ar.get((size_t)n * 8)};
    int *v[2] = {(int *)ar.get((size_t)n * 4), (int *)ar.get((size_t)n * 4)};
    const int ntiles = (int)((n + RX_TILE - 1) / RX_TILE);
    int *hist = (int *)ar.get((size_t)256 * ntiles * 4), *offs = (int *)ar.get((size_t)256 * ntiles * 4);
    int *part = (int *)ar.get((((size_t)256 * ntiles + SCAN_TILE - 1) / SCAN_TILE) * 4);   // one set of tile sums for every pass
    if (ar.rc) return ar.rc;
    const int passes = std::max(1, (bits + 7) / 8);
    const KEY *kin = (const KEY *)d_keys;
    const int *vin = d_vals;
    for (int ps = 0; ps < passes; ps++) {
        KEY *kout = k[ps & 1];
        int *vout = v[ps & 1];
        k_rx_hist<KEY><<<ntiles, 64, 0, ctx->stream>>>(kin, n, 8 * ps, hist, ntiles);
        if (int rc = dev_exclusive_scan<int>(ctx, ar, hist, offs, (int64_t)256 * ntiles, nullptr, nullptr, part)) return rc;
        if (vin) k_rx_scatter<KEY, false><<<ntiles, 64, 0, ctx->stream>>>(kin, vin, n, 8 * ps, offs, ntiles, kout, vout);
        else k_rx_scatter<KEY, true><<<ntiles, 64, 0, ctx->stream>>>(kin, nullptr, n, 8 * ps, offs, ntiles, kout, vout);
        R3D_HIP(ctx, hipGetLastError());
        kin = kout;
        vin = vout;
    }
    *keys_sorted = (const uint64_t *)kin;
    *vals_sorted = vin;
    return R3D_OK;
}

// ================================================================================================ C ABI
// ---- device-pointer cores shared by the host-buffer entry points and the fused device-resident chain -------------

// disparity (device) -> compacted xyz (device).  max_depth > 0 additionally drops points with |z| > max_depth.
// pose4x4 (optional) moves the points; bounds_out[6] (optional) receives their bounding box -- enqueued BEFORE the host knows the
// point count (kernels over the upper bound w * h with the count read on the device), so count and box are ONE read-back.
int reproject_core(r3d_ctx *ctx, DevArena &ar, const int16_t *d_d, int w, int h, const double *Q4x4, int min_valid_x16, double max_depth,
                   bool want_pix, double **d_xyz_out, int **d_pix_out, int64_t *m_out, const double *pose4x4 = nullptr, double *bounds_out = nullptr) {
    const int64_t n = (int64_t)w * h;
    if (n > 0x7fffffff) return r3d_fail(ctx, R3D_E_UNSUPPORTED, "reproject_disparity: image too large");
    int *flags = (int *)ar.get((size_t)n * 4), *scan = (int *)ar.get((size_t)n * 4);
    if (ar.rc) return ar.rc;
    Mat4 Q;
    memcpy(Q.m, Q4x4, sizeof Q.m);
    const int nb = (int)((n + 255) / 256);
    if (max_depth > 0) k_disp_flags_depth<<<nb, 256, 0, ctx->stream>>>(d_d, w, n, min_valid_x16, Q, max_depth, flags);
    else k_disp_flags<<<nb, 256, 0, ctx->stream>>>(d_d, n, min_valid_x16, flags);
    if (int src = dev_exclusive_scan<int>(ctx, ar, flags, scan, n)) return src;
    // With bounds_out the arrays are sized for the upper bound (every pixel valid) and reprojection, pose and bounding box are
    // enqueued before the one read-back; without it the count is read first and the arrays hold exactly the valid pixels.
    const bool upper = bounds_out != nullptr;
    CompactCount cc(scan, flags, n);
    PinRead rd(ctx);
    int rc;
    *m_out = 0;
    *d_xyz_out = nullptr;
    if (d_pix_out) *d_pix_out = nullptr;
    if (!upper) {
        if ((rc = cc.add_to(rd)) || (rc = rd.wait())) return rc;
        if (cc.count() == 0) return R3D_OK;
    }
    const int64_t rows = upper ? n : cc.count();
    double *d_xyz = (double *)ar.get((size_t)rows * 24);
    int *d_pix = want_pix ? (int *)ar.get((size_t)rows * 4) : nullptr;
    if (ar.rc) return ar.rc;
    k_reproject<<<nb, 256, 0, ctx->stream>>>(d_d, flags, scan, w, n, Q, d_xyz, d_pix);
    R3D_HIP(ctx, hipGetLastError());
    if (upper) {
        if (pose4x4) {
            double *d_t = (double *)ar.get((size_t)n * 24);
            if (ar.rc) return ar.rc;
            k_transform_dn<<<nb, 256, 0, ctx->stream>>>(d_xyz, cc.d_scan, cc.d_flag, to_rigid(pose4x4), d_t);
            d_xyz = d_t;
        }
        const double *d_box = nullptr;
        if ((rc = cloud_bbox_enqueue_dn(ctx, ar, d_xyz, n, cc.d_scan, cc.d_flag, &d_box))) return rc;
        if ((rc = cc.add_to(rd)) || (rc = rd.add(bounds_out, d_box, 48)) || (rc = rd.wait())) return rc;
        if (cc.count() == 0) return R3D_OK;
    }
    *m_out = cc.count();
    *d_xyz_out = d_xyz;
    if (d_pix_out) *d_pix_out = d_pix;
    return upper ? bbox_check(ctx, bounds_out, bounds_out + 3) : R3D_OK;
}

// depth image (host) -> compacted xyz / colours (device); everything below r3d_backproject_depth's argument checks
int backproject_core(r3d_ctx *ctx, DevArena &ar, const uint16_t *depth, int w, int h, int stride, const r3d_depth_camera *cam,
                     const uint8_t *color, int cstride, bool want_pix, double **d_xyz_out, double **d_rgb_out, int **d_pix_out, int64_t *m_out,
                     double *bounds_out = nullptr /* [6]: the cloud's bounding box, read back together with the count */,
                     const PinExtra *extra = nullptr /* rides along in that read-back */) {
    const int64_t n = (int64_t)w * h;
    if (n > 0x7fffffff) return r3d_fail(ctx, R3D_E_UNSUPPORTED, "backproject_depth: image too large");
    unsigned short *d_d = (unsigned short *)ar.get((size_t)stride * h * 2);
    unsigned char *d_c = color ? (unsigned char *)ar.get((size_t)cstride * h) : nullptr;
    int *flags = (int *)ar.get((size_t)n * 4), *scan = (int *)ar.get((size_t)n * 4);
    if (ar.rc) return ar.rc;
    // the caller's last row need not be padded to the stride: (h-1) full strides + w elements is all that is guaranteed readable
    R3D_HIP(ctx, hipMemcpyAsync(d_d, depth, ((size_t)stride * (h - 1) + w) * 2, hipMemcpyHostToDevice, ctx->stream));
    if (color) R3D_HIP(ctx, hipMemcpyAsync(d_c, color, (size_t)cstride * (h - 1) + (size_t)w * 3, hipMemcpyHostToDevice, ctx->stream));
    DepthCam c{cam->fx, cam->fy, cam->ppx, cam->ppy, cam->depth_trunc, (float)cam->depth_scale, cam->flip_yz};
    const int nb = (int)((n + 255) / 256);
    k_depth_flags<<<nb, 256, 0, ctx->stream>>>(d_d, w, stride, n, c, flags);
    if (int src = dev_exclusive_scan<int>(ctx, ar, flags, scan, n)) return src;
    // as reproject_core: with bounds_out, arrays for the upper bound and back-projection and bounding box enqueued before the ONE
    // read-back; without it, the count first
    const bool upper = bounds_out != nullptr;
    CompactCount cc(scan, flags, n);
    PinRead rd(ctx);
    int rc;
    *m_out = 0;
    *d_xyz_out = nullptr;
    if (d_rgb_out) *d_rgb_out = nullptr;
    if (d_pix_out) *d_pix_out = nullptr;
    if (!upper) {
        if ((rc = cc.add_to(rd)) || (rc = rd.wait())) return rc;
        if (cc.count() == 0) return R3D_OK;
    }
    const int64_t rows = upper ? n : cc.count();
    double *d_xyz = (double *)ar.get((size_t)rows * 24), *d_rgb = color ? (double *)ar.get((size_t)rows * 24) : nullptr;
    int *d_pix = want_pix ? (int *)ar.get((size_t)rows * 4) : nullptr;
    if (ar.rc) return ar.rc;
    k_backproject<<<nb, 256, 0, ctx->stream>>>(d_d, d_c, flags, scan, w, stride, cstride, n, c, d_xyz, d_rgb, d_pix);
    R3D_HIP(ctx, hipGetLastError());
    if (upper) {
        const double *d_box = nullptr;
        if ((rc = cloud_bbox_enqueue_dn(ctx, ar, d_xyz, n, cc.d_scan, cc.d_flag, &d_box))) return rc;
        if ((rc = cc.add_to(rd)) || (rc = rd.add(bounds_out, d_box, 48)) ||
            (extra && extra->host && (rc = rd.add(extra->host, extra->dev, extra->bytes))) || (rc = rd.wait())) return rc;
        if (cc.count() == 0) return R3D_OK;
    }
    *m_out = cc.count();
    *d_xyz_out = d_xyz;
    if (d_rgb_out) *d_rgb_out = d_rgb;
    if (d_pix_out) *d_pix_out = d_pix;
    return upper ? bbox_check(ctx, bounds_out, bounds_out + 3) : R3D_OK;
}
static int depth_args_ok(r3d_ctx *ctx, const uint16_t *depth, int w, int h, int stride, const r3d_depth_camera *cam, const uint8_t *color,
                         int cstride, const char *who) {
    if (!depth || !cam || w <= 0 || h <= 0 || stride < w || (color && cstride < 3 * w)) return r3d_fail(ctx, R3D_E_BADARG, "%s: bad argument", who);
    if (!(cam->fx != 0) || !(cam->fy != 0) || !(cam->depth_scale > 0) || !(cam->depth_trunc > 0))
        return r3d_fail(ctx, R3D_E_BADARG, "%s: focal lengths must be non-zero, depth_scale and depth_trunc positive", who);
    return R3D_OK;
}
// argument checks of the registration modes P2P / P2PLANE / GICP.  have_tn / have_sn: the caller has, or will compute, target /
// source normals; no_tn: what to say where the plane and GICP modes find none for the target
static int icp_mode_check(r3d_ctx *ctx, const char *who, const r3d_icp_params *p, bool have_tn, bool have_sn,
                          const char *no_tn = "target normals required for this mode") {
    if (p->mode < 0 || p->mode > 2) return r3d_fail(ctx, R3D_E_BADARG, "%s: mode must be 0 (P2P), 1 (P2PLANE) or 2 (GICP)", who);
    if (!(p->max_correspondence_distance > 0)) return r3d_fail(ctx, R3D_E_BADARG, "%s: max_correspondence_distance must be > 0", who);
    if (p->mode != MODE_P2P && !have_tn) return r3d_fail(ctx, R3D_E_BADARG, "%s: %s", who, no_tn);
    if (p->mode == MODE_GICP && !have_sn) return r3d_fail(ctx, R3D_E_BADARG, "%s: source normals required for GICP", who);
    return R3D_OK;
}

// voxel grid of a device cloud: segments of equal legacy voxel index, in lexicographic index order
struct VoxelSegs {
    int *idx = nullptr, *starts = nullptr;
    double *sorted = nullptr;   // the points in (voxel, index) order (written by the sort)
    int64_t nseg = 0;
};
// fixed_org / fixed_max (legacy grid only): use this origin and size the key space for points up to fixed_max instead of deriving
// both from the cloud's own bounding box (the incremental model table: a slice of the model keyed in the MODEL's grid; no
// bounding-box pass).  bounds_out[6] receives min / max of the cloud when its box was computed here.
// known_bounds[6] (min, max of exactly these points, already on the host): no bounding-box pass, same grid.
int voxel_segments(r3d_ctx *ctx, DevArena &ar, const double *d_p, int64_t n, double voxel, VoxelSegs &V, bool tensor_grid = false,
                   const double *fixed_org = nullptr, const double *fixed_max = nullptr, double *bounds_out = nullptr,
                   const double *known_bounds = nullptr) {
    double mn[3], mx[3];
    int rc;
    if (fixed_org) {
        for (int a = 0; a < 3; a++) { mn[a] = fixed_org[a] + 0.5 * voxel; mx[a] = fixed_max[a]; }
    } else if (known_bounds) {
        for (int a = 0; a < 3; a++) { mn[a] = known_bounds[a]; mx[a] = known_bounds[3 + a]; }
        if (bounds_out) for (int a = 0; a < 6; a++) bounds_out[a] = known_bounds[a];
    } else {
        if ((rc = cloud_bbox(ctx, ar, d_p, n, mn, mx))) return rc;
        if (bounds_out) for (int a = 0; a < 3; a++) { bounds_out[a] = mn[a]; bounds_out[3 + a] = mx[a]; }
    }
    double org[3];
    int dims[3];
    double total = 1;
    for (int a = 0; a < 3; a++) {
        if (tensor_grid) {   // o3d.t: key = floor(float(p) / float(voxel)), origin 0; float division by a positive constant is monotonic
            const double k0 = std::floor((float)mn[a] / (float)voxel), k1 = std::floor((float)mx[a] / (float)voxel);
            if (!(std::fabs(k0) < 9e15 && std::fabs(k1) < 9e15 && k1 - k0 < 2.0e9)) return r3d_fail(ctx, R3D_E_UNSUPPORTED, "voxel_downsample: voxel grid too fine for the extent of the cloud");
            org[a] = k0;
            dims[a] = (int)(k1 - k0) + 1;
        } else {
            org[a] = fixed_org ? fixed_org[a] : mn[a] - 0.5 * voxel;  // legacy: voxel_min_bound = min_bound - voxel_size * 0.5
            dims[a] = (int)std::floor((mx[a] - org[a]) / voxel) + 2;
        }
        total *= dims[a];
    }
    if (total >= 1.8e19) return r3d_fail(ctx, R3D_E_UNSUPPORTED, "voxel_downsample: voxel grid exceeds 2^64 cells");
    void *keys;
    bool keys32;
    // key_order 1: exact legacy index floor((p - origin) / voxel), z fastest => output in lexicographic (kx,ky,kz) order
    V.sorted = (double *)ar.get((size_t)n * 24);
    if (ar.rc) return ar.rc;
    // The sort's own round trip (run count + fallback test) is deferred and travels with the segment count: ONE read-back for the
    // whole voxel grid.  If the test then says the counting sort had to decline (rare: thousands of runs in one bucket), the
    // arrays are garbage: sort again with the library radix sort and repeat the segmentation.
    int *flags = (int *)ar.get((size_t)n * 4), *scan = (int *)ar.get((size_t)n * 4);
    V.starts = (int *)ar.get((size_t)n * 4);
    if (ar.rc) return ar.rc;
    const int nb = (int)((n + 255) / 256);
    for (int attempt = 0; attempt < 2; attempt++) {
        SortDefer df;
        if ((rc = sort_by_cell(ctx, ar, d_p, n, org, voxel, dims, tensor_grid ? 3 : 1, &keys, &keys32, &V.idx, V.sorted, attempt ? 1 : -1,
                               attempt ? nullptr : &df))) return rc;
        with_keys(keys32, keys, [&](auto *k) { k_seg_flags<<<nb, 256, 0, ctx->stream>>>(k, n, flags); });
        if (int src = dev_exclusive_scan<int>(ctx, ar, flags, scan, n)) return src;
        k_seg_starts<<<nb, 256, 0, ctx->stream>>>(flags, scan, n, V.starts);
        CompactCount cc(scan, flags, n);
        PinRead rd(ctx);
        if ((rc = cc.add_to(rd)) || (rc = df.add_to(rd)) || (rc = rd.wait())) return rc;
        V.nseg = cc.count();
        if (df.ok()) return R3D_OK;
        static const bool dbg = [] { const char *e = getenv("R3D_SORT_DEBUG"); return e && *e == '1'; }();
        if (dbg) fprintf(stderr, "[r3d sort] voxel grid: deferred test failed (n=%lld runs=%d max_runs_per_bucket=%d): sorting again with the radix sort\n",
                         (long long)n, (int)(df.h_total >> 32), df.h_maxruns);
    }
    return r3d_fail(ctx, R3D_E_HIP, "voxel grid: the fallback sort did not complete");
}
// Voxel-down-sampled points of a device cloud: the means of the voxels' members, V.nseg rows in a fresh arena buffer.
// tensor_grid / bounds_out / known_bounds: voxel_segments'.  V stays valid for voxel_attr_means and for readers of the sorted points.
int voxel_means(r3d_ctx *ctx, DevArena &ar, const double *d_p, int64_t n, double voxel, VoxelSegs &V, double **d_means, bool tensor_grid = false,
                double *bounds_out = nullptr, const double *known_bounds = nullptr) {
    if (int rc = voxel_segments(ctx, ar, d_p, n, voxel, V, tensor_grid, nullptr, nullptr, bounds_out, known_bounds)) return rc;
    *d_means = (double *)ar.get((size_t)V.nseg * 24);
    if (ar.rc) return ar.rc;
    return launch_voxel_mean(ctx, ar, tensor_grid, d_p, V.idx, V.starts, V.nseg, n, *d_means, V.sorted);
}
// a further attribute of the same n points (colours, normals: [n][3], the cloud's order) averaged over the same voxels
int voxel_attr_means(r3d_ctx *ctx, DevArena &ar, const VoxelSegs &V, const double *d_a, int64_t n, double **d_means, bool f32 = false) {
    *d_means = (double *)ar.get((size_t)V.nseg * 24);
    if (ar.rc) return ar.rc;
    return launch_voxel_mean(ctx, ar, f32, d_a, V.idx, V.starts, V.nseg, n, *d_means);
}

// Launch of a kernel that keeps its k nearest neighbours in LDS columns (knn_collect): one thread per point, k * 12 bytes of dynamic
// LDS each.  Every such kernel's parameters begin (grid, n, k, radius); `rest` are the others.
template <class... P, class... A>
int launch_knn(r3d_ctx *ctx, void (*kernel)(GridView, int64_t, int, double, P...), const Grid &G, int64_t n, int k, double radius, A... rest) {
    const size_t lds = (size_t)k * KNN_BLOCK * 12;
    R3D_HIP(ctx, hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    kernel<<<(unsigned)((n + KNN_BLOCK - 1) / KNN_BLOCK), KNN_BLOCK, lds, ctx->stream>>>(G.v, n, k, radius, rest...);
    R3D_HIP(ctx, hipGetLastError());
    return R3D_OK;
}
// occupied cells of a k-NN search grid should hold about this many points (grid_build's target_occ)
inline double knn_target_occ(int k) { return std::max(2.0, k / 5.0); }
// ... unless R3D_KNN_OCC says otherwise (normals and colour gradients only)
inline double knn_target_occ_env(int k) {
    if (const char *oe = getenv("R3D_KNN_OCC")) { const double v = atof(oe); if (v >= 0.5 && v <= 256) return v; }
    return knn_target_occ(k);
}

// normals of a device cloud into a fresh device buffer
int normals_core(r3d_ctx *ctx, DevArena &ar, const double *d_p, int64_t n, double radius, int max_nn, const double *d_prev, double **d_n_out,
                 const double *enclosing = nullptr) {
    Grid G;
    const int k = (int)std::min<int64_t>(max_nn, n);
    int rc;
    if ((rc = grid_build(ctx, ar, d_p, n, radius, knn_target_occ_env(k), G, false, enclosing))) return rc;
    double *d_n = (double *)ar.get((size_t)n * 24);
    if (ar.rc) return ar.rc;
    *d_n_out = d_n;
    return launch_knn(ctx, k_normals, G, n, k, radius, d_prev, d_n, nullptr);
}

// intensity + colour gradient of a device cloud (k_color_gradient's 4-double records, the caller's numbering) into a fresh device
// buffer; the search grid follows normals_core's rule
int color_gradients_core(r3d_ctx *ctx, DevArena &ar, const double *d_p, int64_t n, const double *d_n, const double *d_c, double radius, int max_nn,
                         double **d_rec_out) {
    Grid G;
    const int k = (int)std::min<int64_t>(max_nn, n);
    int rc;
    if ((rc = grid_build(ctx, ar, d_p, n, radius, knn_target_occ_env(k), G, false))) return rc;
    double *d_i = (double *)ar.get((size_t)n * 8), *d_rec = (double *)ar.get((size_t)n * 32);
    if (ar.rc) return ar.rc;
    k_intensity<<<(unsigned)((n + 255) / 256), 256, 0, ctx->stream>>>(d_c, G.v.idx, n, d_i);
    *d_rec_out = d_rec;
    return launch_knn(ctx, k_color_gradient, G, n, k, radius, d_n, d_i, d_rec);
}

// FPFH of a device cloud into the caller's device arrays d_fpfh / d_spfh_out ([n][33], the caller's numbering; d_spfh_out may be
// null).  d_n == null: the second stage alone on d_spfh_in (the caller's numbering).  Nothing waits for the stream beyond the
// grid's own bounding-box read.  The neighbour lists are STORED by the first stage (12 B x (k - 1) per point, written and read
// once: 2.4 GB of traffic at 1 M points and k = 100) rather than searched a second time.
// ev (optional, 3 events): recorded before the first stage, between the stages and after the second (tools/gpu_bench_fpfh.py).
int fpfh_core(r3d_ctx *ctx, DevArena &ar, const double *d_p, const double *d_n, const double *d_spfh_in, int64_t n, double radius, int max_nn,
              double *d_fpfh, double *d_spfh_out, hipEvent_t *ev = nullptr) {
    Grid G;
    const int k = (int)std::min<int64_t>(max_nn, n);
    int rc;
    if ((rc = grid_build(ctx, ar, d_p, n, radius, knn_target_occ(k), G))) return rc;
    const size_t slots = (size_t)std::max(k - 1, 1);
    int *l_cnt = (int *)ar.get((size_t)n * 4), *l_idx = (int *)ar.get(slots * n * 4);
    double *l_d2 = (double *)ar.get(slots * n * 8), *spfh_s = (double *)ar.get((size_t)n * FPFH_DIM * 8);
    double *nrm_s = d_n ? (double *)ar.get((size_t)n * 24) : nullptr;
    if (ar.rc) return ar.rc;
    if (ev) R3D_HIP(ctx, hipEventRecord(ev[0], ctx->stream));
    if (d_n) {
        k_gather3<<<(unsigned)((n + 255) / 256), 256, 0, ctx->stream>>>(d_n, G.v.idx, n, nrm_s);
        rc = launch_knn(ctx, k_spfh, G, n, k, radius, nrm_s, l_cnt, l_idx, l_d2, spfh_s, d_spfh_out);
    } else {
        k_gather_rows33<<<(unsigned)((n * FPFH_DIM + 255) / 256), 256, 0, ctx->stream>>>(d_spfh_in, G.v.idx, n, spfh_s);
        rc = launch_knn(ctx, k_fpfh_lists, G, n, k, radius, l_cnt, l_idx, l_d2);
    }
    if (rc) return rc;
    if (ev) R3D_HIP(ctx, hipEventRecord(ev[1], ctx->stream));
    k_fpfh<<<(unsigned)((n + KNN_BLOCK - 1) / KNN_BLOCK), 64, 0, ctx->stream>>>(n, l_cnt, l_idx, l_d2, spfh_s, G.v.idx, d_fpfh);
    R3D_HIP(ctx, hipGetLastError());
    if (ev) R3D_HIP(ctx, hipEventRecord(ev[2], ctx->stream));
    return R3D_OK;
}

// brute-force matching costs ns * nt * 99 float64 operations: 39 ms per 10^10 pairs measured on the MI355X (profiles/fpfh.json), so
// one call at this product runs for about a minute; beyond it the call is refused
constexpr double MATCH_MAX_PAIRS = 1.5e13;
int match_core(r3d_ctx *ctx, DevArena &ar, const double *d_src, int64_t ns, const double *d_tgt, int64_t nt, int *d_nn, double *d_d2) {
    // the targets are cut into shares so that a small source set still fills the chip (about 2048 workgroups)
    const int64_t tiles = (nt + MATCH_TILE - 1) / MATCH_TILE, nbs = (ns + MATCH_BLOCK - 1) / MATCH_BLOCK;
    const int64_t want = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(tiles, 2048 / nbs), 65535));
    const int64_t per = (tiles + want - 1) / want;
    const int shares = (int)((tiles + per - 1) / per);
    double *p_d2 = (double *)ar.get((size_t)shares * ns * 8);
    int *p_idx = (int *)ar.get((size_t)shares * ns * 4);
    if (ar.rc) return ar.rc;
    k_match_features<<<dim3((unsigned)nbs, (unsigned)shares), MATCH_BLOCK, 0, ctx->stream>>>(d_src, ns, d_tgt, nt, per, p_d2, p_idx);
    k_match_reduce<<<(unsigned)((ns + 255) / 256), 256, 0, ctx->stream>>>(p_d2, p_idx, ns, shares, d_nn, d_d2);
    R3D_HIP(ctx, hipGetLastError());
    return R3D_OK;
}

// the coloured mode's extra inputs (device colours of both clouds) and parameters, resolved by the entry point
struct IcpColorInput { const double *d_sc, *d_tc; double lambda, radius; int max_nn; };
// What a registration runs on: clouds that are already in device memory (d_sn / d_tn may be null where the mode allows it).
// The call sites name what they set; the rest is zero.
struct IcpInput {
    const double *d_s; int64_t ns; const double *d_sn;   // the source and its normals
    const double *d_t; int64_t nt; const double *d_tn;   // the target and its normals
    const double *init4x4;         // the initial pose (null: the identity)
    const double *tgt_enclosing;   // optional: grid_build's `enclosing`
    double tgt_spacing;            // optional: grid_build's `spacing_hint`, the voxel size the target was down-sampled with
    const IcpColorInput *color;    // MODE_COLORED (and only then)
};
// What icp_setup leaves for the evaluations, the loop and the two read-outs (the device buffers belong to the call's arena)
struct IcpWork {
    Grid G;                            // the target's search grid (G.v) and its box
    IcpOrigin org;                     // the point the point-to-point slots are relative to: the centre of that box
    int64_t ns;
    double *d_s, *d_sn, *d_tns;        // the source and its normals in Morton order, the target's normals in cell-sorted order
    int *sidx;                         // the permutation that sorted the source
    IcpColor colk;
    const double *d_trec;              // MODE_COLORED: the target's records in the caller's numbering (colk.tgt_ig before k_gather4), else null
    double *d_part;
    IcpState *d_st, *hst, *d_mirror;   // hst is pinned and mapped: k_icp_step publishes the state there (d_mirror), the host polls it
    int nblocks, search;
};

// The search form of a registration's evaluations.  The default is the packed search (nn_block_q10).  Its cell-relative
// quantisation needs (p - origin) / cell exact to well below 1/1024: a cloud whose coordinates are that large against its cell
// keeps the all-float64 search (nn_block_global), and R3D_ICP_IMPL=exact asks for it on any cloud (the tests' oracle); any other
// value is ignored.  Of the packed forms, small source clouds (at most two workgroups per CU: every gather of the scan is a full
// round trip) take the one that keeps three candidate groups in flight; R3D_ICP_DEEP=0 / 1 forces either form (A/B)
static int icp_search_form(const Grid &G, double max_dist, int64_t ns, int cus) {
    static const int deep_env = [] { const char *e = getenv("R3D_ICP_DEEP"); return !e ? -1 : atoi(e) != 0; }();
    const char *ie = getenv("R3D_ICP_IMPL");
    const bool want_exact = ie && strcmp(ie, "exact") == 0;
    double M = 0;
    for (int a = 0; a < 3; a++) M = std::max(M, std::max(std::fabs(G.mn[a]), std::fabs(G.mx[a])));
    const double Mq = M + 2.0 * max_dist + G.v.cell;
    if (want_exact || !(Mq / G.v.cell < 1e9)) return SEARCH_EXACT;
    const bool deep_search = deep_env >= 0 ? deep_env == 1 : ns <= (int64_t)ICP_BLOCK * std::max(cus, 1) * 2;
    return deep_search ? SEARCH_Q10_DEEP : SEARCH_Q10;
}

// Set-up of a registration: everything between the entry point's argument checks and uploads and the first evaluation
static int icp_setup(r3d_ctx *ctx, DevArena &ar, const r3d_icp_params *p, const IcpInput &in, IcpWork &w) {
    const int64_t ns = in.ns, nt = in.nt;
    const IcpColorInput *const color = in.color;
    Grid &G = w.G;
    int rc;
    // coloured mode: the target's intensities and gradients, once per call (a search grid of its own: the radius differs)
    double *d_trec = nullptr;
    if (color && (rc = color_gradients_core(ctx, ar, in.d_t, nt, in.d_tn, color->d_tc, color->radius, color->max_nn, &d_trec))) return rc;
    w.d_trec = d_trec;
    double occ = 3.0;   // points per occupied cell the search grid aims at (R3D_ICP_OCC: A/B)
    if (const char *oe = getenv("R3D_ICP_OCC")) { const double v = atof(oe); if (v >= 0.5 && v <= 64) occ = v; }
    if ((rc = grid_build(ctx, ar, in.d_t, nt, p->max_correspondence_distance, occ, G, true, in.tgt_enclosing, in.tgt_spacing))) return rc;   // dense table: one load per row in the loop
    int cus = 256;
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device);
    w.search = icp_search_form(G, p->max_correspondence_distance, ns, cus);
    if (w.search != SEARCH_EXACT) {   // packed copy of the target for nn_block_q10
        unsigned *q = (unsigned *)ar.get((size_t)(nt + 4) * sizeof(unsigned));
        if (ar.rc) return ar.rc;
        G.v.q10 = q;
        G.v.pool = 1;
        k_pack_q10<<<(unsigned)((nt + 4 + 255) / 256), 256, 0, ctx->stream>>>(G.v, nt, q);
        R3D_HIP(ctx, hipGetLastError());
    }
    w.d_tns = nullptr;
    if (in.d_tn) {
        w.d_tns = (double *)ar.get((size_t)nt * 24);
        if (ar.rc) return ar.rc;
        k_gather3<<<(unsigned)((nt + 255) / 256), 256, 0, ctx->stream>>>(in.d_tn, G.v.idx, nt, w.d_tns);
    }
    w.colk = {};
    if (color) {
        double *d_trecs = (double *)ar.get((size_t)nt * 32);
        if (ar.rc) return ar.rc;
        k_gather4<<<(unsigned)((nt + 255) / 256), 256, 0, ctx->stream>>>(d_trec, G.v.idx, nt, d_trecs);
        w.colk.tgt_ig = d_trecs;
        w.colk.sg = std::sqrt(color->lambda);
        w.colk.sp = std::sqrt(1.0 - color->lambda);
    }
    // spatially sort the source once (Morton order of the target-grid cell of its initial pose) so that neighbouring threads
    // walk the same cells; sums are order-dependent only at the 1e-16 level and stay deterministic
    double T[16];
    if (in.init4x4) memcpy(T, in.init4x4, sizeof T);
    else for (int i = 0; i < 16; i++) T[i] = (i % 5 == 0);
    double *d_s0 = (double *)ar.get((size_t)ns * 24);
    if (ar.rc) return ar.rc;
    k_transform<<<(unsigned)((ns + 255) / 256), 256, 0, ctx->stream>>>(in.d_s, ns, to_rigid(T), 0, d_s0);
    int dims[3] = {G.v.nx, G.v.ny, G.v.nz};
    void *sk;
    bool sk32;
    if ((rc = sort_by_cell(ctx, ar, d_s0, ns, G.mn, G.v.cell, dims, 2, &sk, &sk32, &w.sidx))) return rc;
    w.d_s = (double *)ar.get((size_t)ns * 24);
    if (ar.rc) return ar.rc;
    k_gather3<<<(unsigned)((ns + 255) / 256), 256, 0, ctx->stream>>>(in.d_s, w.sidx, ns, w.d_s);
    w.d_sn = nullptr;
    if (in.d_sn) {
        w.d_sn = (double *)ar.get((size_t)ns * 24);
        if (ar.rc) return ar.rc;
        k_gather3<<<(unsigned)((ns + 255) / 256), 256, 0, ctx->stream>>>(in.d_sn, w.sidx, ns, w.d_sn);
    }
    if (color) {
        double *d_si = (double *)ar.get((size_t)ns * 8);
        if (ar.rc) return ar.rc;
        k_intensity<<<(unsigned)((ns + 255) / 256), 256, 0, ctx->stream>>>(color->d_sc, w.sidx, ns, d_si);
        w.colk.src_i = d_si;
    }
    // one residency of the chip (3 workgroups per CU at the kernel's register count): every wave starts at once, walks its share
    // of the queries in a grid-stride loop and pays the 29-slot reduction once
    w.ns = ns;
    w.nblocks = (int)std::min<int64_t>((ns + ICP_BLOCK - 1) / ICP_BLOCK, (int64_t)std::max(cus, 1) * 3);
    w.d_part = (double *)ar.get((size_t)w.nblocks * ICP_SLOTS * 8);
    w.d_st = (IcpState *)ar.get(sizeof(IcpState));
    if (ar.rc) return ar.rc;
    static_assert(sizeof(IcpState) <= ICP_SLOTS * sizeof(double), "the pinned landing buffer holds one IcpState");
    if (!ctx->icp_host.p) R3D_HIP(ctx, ctx->icp_host.alloc(ICP_SLOTS * sizeof(double), hipHostMallocMapped));
    w.hst = (IcpState *)ctx->icp_host.p;   // pinned and mapped: k_icp_step publishes the state here, the host polls it
    w.d_mirror = nullptr;
    R3D_HIP(ctx, hipHostGetDevicePointer((void **)&w.d_mirror, w.hst, 0));
    memset(w.hst, 0, sizeof *w.hst);
    memcpy(w.hst->T, T, sizeof T);
    R3D_HIP(ctx, hipMemcpyAsync(w.d_st, w.hst, sizeof *w.hst, hipMemcpyHostToDevice, ctx->stream));
    // what the point-to-point moments are relative to: a fixed point both clouds are near (the paired sources lie within the
    // distance of the target's box)
    w.org = {0.5 * (G.mn[0] + G.mx[0]), 0.5 * (G.mn[1] + G.mx[1]), 0.5 * (G.mn[2] + G.mx[2])};
    return R3D_OK;
}

// one evaluation of the loop, enqueued without waiting (it returns at once when the loop has ended): one kernel per search form x
// mode.  `corr`: the kernel's optional output (the read-outs'; the loop passes nullptr)
static void icp_enqueue_eval(r3d_ctx *ctx, const r3d_icp_params *p, const IcpWork &w, int *corr) {
    const double eps = p->gicp_epsilon > 0 ? p->gicp_epsilon : 1e-3;
    const double md = p->max_correspondence_distance;
    with_const<SEARCH_Q10_DEEP, SEARCH_Q10, SEARCH_EXACT>(w.search, [&](auto search) {
        with_const<MODE_P2P, MODE_P2PLANE, MODE_COLORED, MODE_GICP>(p->mode, [&](auto mode) {
            k_icp_eval<decltype(mode)::value, decltype(search)::value><<<w.nblocks, ICP_BLOCK, 0, ctx->stream>>>(
                w.G.v, w.d_s, w.d_sn, w.d_tns, w.ns, w.d_st, md, eps, w.d_part, corr, w.colk, w.org);
        });
    });
}

// r3d_debug_icp_sums' read-out (host: sums [29], origin [3] or null): the loop's own evaluation, then k_icp_step's reduction of
// its partial sums
static int icp_read_sums(r3d_ctx *ctx, DevArena &ar, const r3d_icp_params *p, const IcpWork &w, double *sums, double *origin) {
    int *d_corr = (int *)ar.get((size_t)w.ns * 4);
    double *d_sums = (double *)ar.get(ICP_SLOTS * 8);
    if (ar.rc) return ar.rc;
    icp_enqueue_eval(ctx, p, w, d_corr);
    k_icp_sums_readout<<<1, 1024, 0, ctx->stream>>>(w.d_part, w.nblocks, d_sums);
    R3D_HIP(ctx, hipGetLastError());
    if (int rc = r3d_download(ctx, sums, d_sums, ICP_SLOTS)) return rc;
    R3D_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (origin) { origin[0] = w.org.x; origin[1] = w.org.y; origin[2] = w.org.z; }
    return R3D_OK;
}
// r3d_debug_icp_correspondences' read-out (host arrays in the caller's numbering, d2 may be null): one evaluation at the initial
// pose; d_t is the target in the caller's order
static int icp_read_correspondences(r3d_ctx *ctx, DevArena &ar, const r3d_icp_params *p, const IcpWork &w, const double *d_t, int32_t *corr,
                                    double *d2) {
    const int64_t ns = w.ns;
    int *d_corr = (int *)ar.get((size_t)ns * 4), *d_corr_out = (int *)ar.get((size_t)ns * 4);
    double *d_d2_out = (double *)ar.get((size_t)ns * 8);
    if (ar.rc) return ar.rc;
    icp_enqueue_eval(ctx, p, w, d_corr);
    k_icp_corr_readout<<<(unsigned)((ns + 255) / 256), 256, 0, ctx->stream>>>(w.d_s, w.sidx, ns, w.d_st, d_t, d_corr, d_corr_out, d_d2_out);
    R3D_HIP(ctx, hipGetLastError());
    int rc;
    if ((rc = r3d_download(ctx, corr, d_corr_out, (size_t)ns)) || (rc = r3d_download(ctx, d2, d_d2_out, (size_t)ns))) return rc;
    R3D_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return R3D_OK;
}

// Bounded wait for the state k_icp_step publishes in the mapped host buffer (`seq` reaches `need`, or the DONE bit: `loop_done`).  A
// tight spin for the first 200 us (a batch of a small cloud is shorter than a sleep), then the thread yields between
// polls.  The deadline scales with the work enqueued (serialised counter passes are ~100x slower than a plain run); on
// expiry the call fails with the last state read so the caller exits non-zero.
static int icp_poll(r3d_ctx *ctx, const IcpState *hst, int need, int enq, double deadline_s, bool &loop_done) {
    const auto t_poll = std::chrono::steady_clock::now();
    for (unsigned spins = 0;; spins++) {
        // `seq` is the last word k_icp_step stores, behind a system-scope fence: once it shows the awaited step, or the
        // DONE bit, every other field of that step is visible
        const int seq = *(volatile const int *)&hst->seq;
        std::atomic_thread_fence(std::memory_order_acquire);
        if ((seq & ~ICP_SEQ_DONE) >= need || (seq & ICP_SEQ_DONE)) { loop_done = (seq & ICP_SEQ_DONE) != 0; return R3D_OK; }
        if ((spins & 63) != 63) continue;
        const double waited = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_poll).count();
        if (waited > deadline_s) {
            ctx->poisoned = true;   // the batch is still queued on arena buffers: no later call may reuse them
            return r3d_fail(ctx, R3D_E_HIP, "registration loop: no completion after %.0f s (%d evaluations enqueued, last state read: %d evaluations, done=%d)",
                            waited, enq, hst->evals, hst->done);
        }
        if (waited > 2e-4) std::this_thread::sleep_for(std::chrono::microseconds(waited > 5e-3 ? 200 : 20));
    }
}

// The loop of a registration on icp_setup's work record: the final pose to T4x4, the loop's figures to `stats` (may be null)
static int icp_loop(r3d_ctx *ctx, const r3d_icp_params *p, const IcpWork &w, int64_t nt, double *T4x4, r3d_icp_stats *stats,
                    std::chrono::steady_clock::time_point t_begin) {
    const IcpState *const hst = w.hst;
    R3D_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const auto t_loop = std::chrono::steady_clock::now();
    // The loop of RegistrationICP (evaluate, test, update) runs on the device; the host enqueues ICP_BATCH evaluations at a
    // time and reads the state back once per batch (a host round trip per iteration cost ~50 us of a 0.22 ms iteration).
    // The host polls the state that k_icp_step publishes in a mapped host buffer instead of a blocking stream synchronise: the
    // blocking wait may put the thread to sleep for a scheduler tick (occasional 40-50 ms waits).
    // A WINDOW of evaluations stays enqueued: ICP_BATCH at first, then ICP_STRIDE more whenever all but ICP_STRIDE of them have
    // been consumed -- the device never runs dry while the host notices a batch's end and enqueues the next (that hand-over
    // left the GPU idle for ~40 us per 8 iterations: profiles/r04_icp_timeline.txt).  k_icp_step publishes its state to the
    // host mirror only at the steps the host waits for (every ICP_STRIDE-th and the last).
    // Large clouds (an evaluation is >= 50 us) get a window of 24, topped up by 8: the default 20- and 30-iteration loops are then
    // enqueued (almost) whole and do not depend on the host thread being scheduled in time -- the 10-50 ms "device queue not
    // served" loops of shared boxes were the device running dry behind a descheduled host; evaluations behind the step that ends
    // the loop return at their first instruction (at most 24 x ~8 us).  R3D_ICP_WINDOW=<batch> overrides (stride = batch / 2).
    static const int win_env = [] { const char *e = getenv("R3D_ICP_WINDOW"); const int v = e ? atoi(e) : 0; return v < 2 ? 0 : (v > 256 ? 256 : v); }();
    const bool big = w.ns >= 500000;
    const int ICP_BATCH = win_env ? win_env : big ? 24 : 8, ICP_STRIDE = win_env ? std::max(win_env / 2, 1) : big ? 8 : 4;
    const double deadline_s = 20.0 + 2e-6 * (double)(w.ns + nt) * ICP_BATCH;
    bool loop_done = false;
    const int total = p->max_iteration + 1;
    for (int enq = 0; enq < total && !loop_done;) {
        for (int b = 0, nb = enq == 0 ? ICP_BATCH : ICP_STRIDE; b < nb && enq < total; b++, enq++) {
            // a step publishes its state to the host mirror (~20 posted writes and a system-scope fence) only if the host will WAIT
            // for it: the last one, and the steps `need` below names (ICP_BATCH - ICP_STRIDE, then every ICP_STRIDE-th, while more
            // evaluations remain to be enqueued behind them); a step that ENDS the loop publishes by itself
            const int sno = enq + 1, first_need = ICP_BATCH - ICP_STRIDE;
            const bool awaited = sno == total || (sno >= first_need && (sno - first_need) % ICP_STRIDE == 0 && sno + ICP_STRIDE < total);
            icp_enqueue_eval(ctx, p, w, nullptr);   // the evaluation and its step both return at once when the loop has ended
            k_icp_step<<<1, 1024, 0, ctx->stream>>>(w.d_part, w.nblocks, w.d_st, w.ns, p->mode, p->max_iteration, p->relative_fitness, p->relative_rmse,
                                                    w.d_mirror, awaited ? 1 : 0, w.org);
        }
        R3D_HIP(ctx, hipGetLastError());
        // evaluations that must have been consumed before the host goes on: everything at the end, all but the last ICP_STRIDE
        // otherwise
        const int need = enq >= total ? enq : enq - ICP_STRIDE;
        if (int rc = icp_poll(ctx, hst, need, enq, deadline_s, loop_done)) return rc;
    }
    if (!loop_done) return r3d_fail(ctx, R3D_E_HIP, "registration loop did not finish (%d evaluations)", hst->evals);
    // (evaluations enqueued behind the step that ended the loop may still be in flight: they return at their first
    // instruction (`done`), and everything this call or the next enqueues is ordered behind them on the same stream)
    memcpy(T4x4, hst->T, sizeof hst->T);
    if (stats) {
        stats->iterations = hst->iterations;
        stats->converged = hst->converged;
        stats->correspondences = (int64_t)hst->corr;
        stats->fitness = hst->fit;
        stats->inlier_rmse = hst->rmse;
        const auto t_end = std::chrono::steady_clock::now();
        stats->setup_ms = std::chrono::duration<double, std::milli>(t_loop - t_begin).count();
        stats->loop_ms = std::chrono::duration<double, std::milli>(t_end - t_loop).count();
    }
    {
        static const bool dbg = [] { const char *e = getenv("R3D_ICP_DEBUG"); return e && *e == '1'; }();
        if (dbg) {
            const double host_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_loop).count();
            const double dev_ms = (double)(hst->t_last - hst->t_first) * 1e-5;   // 100 MHz ticks, first step to last step
            if (host_ms > 10.0 || host_ms > 5.0 + 3.0 * dev_ms)
                fprintf(stderr, "[r3d icp] loop: host %.3f ms, device first-to-last step %.3f ms (%d evaluations): the device %s\n", host_ms, dev_ms,
                        hst->evals, dev_ms > 0.5 * host_ms ? "itself was stalled" : "finished on time, the completion reached the host late");
        }
    }
    return R3D_OK;
}

// ICP / point-to-plane / GICP / coloured loop on clouds that are already in device memory: everything below r3d_icp's argument
// checks and uploads
static int icp_core(r3d_ctx *ctx, DevArena &ar, const r3d_icp_params *p, const IcpInput &in, double *T4x4, r3d_icp_stats *stats,
                    std::chrono::steady_clock::time_point t_begin) {
    IcpWork w;
    if (int rc = icp_setup(ctx, ar, p, in, w)) return rc;
    return icp_loop(ctx, p, w, in.nt, T4x4, stats, t_begin);
}

// ---- Fast Global Registration: the host side (the kernels stand next to the RANSAC block)
namespace {

int fgr_check(r3d_ctx *ctx, const char *who, const r3d_fgr_params *p, const void *src, int64_t ns, const void *tgt, int64_t nt) {
    if (!p || !src || !tgt || ns < 1 || nt < 1) return r3d_fail(ctx, R3D_E_BADARG, "%s: bad argument (null array or empty cloud)", who);
    if (!(p->division_factor > 1) || !(p->maximum_correspondence_distance > 0) || !(p->tuple_scale > 0) || !(p->tuple_scale <= 1) ||
        !std::isfinite(p->division_factor) || !std::isfinite(p->maximum_correspondence_distance) || p->iteration_number < 0 ||
        p->maximum_tuple_count < 1 || p->batch < 0)
        return r3d_fail(ctx, R3D_E_BADARG, "%s: division_factor > 1, maximum_correspondence_distance > 0, 0 < tuple_scale <= 1, iteration_number >= 0, "
                                           "maximum_tuple_count >= 1 and batch >= 0 are required", who);
    if (ns > 0x7fffffff || nt > 0x7fffffff) return r3d_fail(ctx, R3D_E_UNSUPPORTED, "%s: ns and nt must stay below 2^31", who);
    return R3D_OK;
}

// step 1 of the contract: the means and the largest centred norm of both clouds in two fixed-order two-level passes, one read-back
int fgr_normalise(r3d_ctx *ctx, DevArena &ar, const double *d_src, int64_t ns, const double *d_tgt, int64_t nt, bool absolute, FgrNorm &nm,
                  double *scale_start) {
    const int nb = (int)std::min<int64_t>((std::max(ns, nt) + 255) / 256, FGR_MOM_BLOCKS);
    double *part = (double *)ar.get((size_t)nb * 6 * 8), *part2 = (double *)ar.get((size_t)nb * 2 * 8), *mom = (double *)ar.get(64);
    if (ar.rc) return ar.rc;
    k_fgr_moments<<<dim3(nb, 2), 256, 0, ctx->stream>>>(d_src, ns, d_tgt, nt, part);
    k_fgr_moments_final<<<1, 256, 0, ctx->stream>>>(part, nb, ns, nt, mom);
    k_fgr_maxnorm<<<dim3(nb, 2), 256, 0, ctx->stream>>>(d_src, ns, d_tgt, nt, mom, part2);
    k_fgr_maxnorm_final<<<1, 256, 0, ctx->stream>>>(part2, nb * 2, mom);
    R3D_HIP(ctx, hipGetLastError());
    double h[8];
    PinRead rd(ctx);
    int rc;
    if ((rc = rd.add(h, mom, sizeof h)) || (rc = rd.wait())) return rc;
    const double scale = h[6];
    if (!(scale > 0) || !std::isfinite(scale))
        return r3d_fail(ctx, R3D_E_BADARG, "fgr: the clouds have no extent or non-finite coordinates (largest centred norm %g)", scale);
    for (int a = 0; a < 3; a++) { nm.mean_s[a] = h[a]; nm.mean_t[a] = h[3 + a]; }
    nm.scale_global = absolute ? 1.0 : scale;
    *scale_start = absolute ? scale : 1.0;
    return R3D_OK;
}

// the normalised [M][6] rows of the pairs, their indices checked on the device before anything reads a row
int fgr_gather(r3d_ctx *ctx, DevArena &ar, const double *d_src, int64_t ns, const double *d_tgt, int64_t nt, const int *d_corres, int64_t M,
               const FgrNorm &nm, double **rows_out) {
    double *rows = (double *)ar.get((size_t)M * 48);
    int *d_bad = (int *)ar.get(4);
    if (ar.rc) return ar.rc;
    *rows_out = rows;
    if (M == 0) return R3D_OK;
    R3D_HIP(ctx, hipMemsetAsync(d_bad, 0, 4, ctx->stream));
    k_fgr_gather<<<(unsigned)((M + 255) / 256), 256, 0, ctx->stream>>>(d_src, ns, d_tgt, nt, d_corres, M, nm, rows, d_bad);
    R3D_HIP(ctx, hipGetLastError());
    int bad = 0, rc;
    PinRead rd(ctx);
    if ((rc = rd.add(&bad, d_bad, 4)) || (rc = rd.wait())) return rc;
    if (bad) return r3d_fail(ctx, R3D_E_BADARG, "fgr: a correspondence index lies outside its cloud (ns = %lld, nt = %lld)", (long long)ns, (long long)nt);
    return R3D_OK;
}

// step 2, feature form: both searches, the cross-check, the pairs compacted in ascending source index; one read-back (the count)
int fgr_mutual(r3d_ctx *ctx, DevArena &ar, const double *d_sf, int64_t ns, const double *d_tf, int64_t nt, int **corres_out, int64_t *M_out,
               double ms[2] /* matching, filter: filled when timing */, bool timing) {
    int *nn_st = (int *)ar.get((size_t)ns * 4), *nn_ts = (int *)ar.get((size_t)nt * 4);
    int *flag = (int *)ar.get((size_t)(ns + 1) * 4), *scan = (int *)ar.get((size_t)(ns + 1) * 4), *corres = (int *)ar.get((size_t)ns * 8);
    if (ar.rc) return ar.rc;
    int rc;
    auto t0 = std::chrono::steady_clock::now();
    if ((rc = match_core(ctx, ar, d_sf, ns, d_tf, nt, nn_st, nullptr))) return rc;
    if ((rc = match_core(ctx, ar, d_tf, nt, d_sf, ns, nn_ts, nullptr))) return rc;
    if (timing) {
        R3D_HIP(ctx, hipStreamSynchronize(ctx->stream));
        const auto t1 = std::chrono::steady_clock::now();
        ms[0] = std::chrono::duration<double, std::milli>(t1 - t0).count();
        t0 = t1;
    }
    k_fgr_mutual<<<(unsigned)((ns + 1 + 255) / 256), 256, 0, ctx->stream>>>(nn_st, ns, nn_ts, nt, flag);
    R3D_HIP(ctx, hipGetLastError());
    if ((rc = dev_exclusive_scan<int>(ctx, ar, flag, scan, ns + 1))) return rc;
    k_fgr_mutual_compact<<<(unsigned)((ns + 255) / 256), 256, 0, ctx->stream>>>(nn_st, ns, flag, scan, corres);
    R3D_HIP(ctx, hipGetLastError());
    int count = 0;
    PinRead rd(ctx);
    if ((rc = rd.add(&count, scan + ns, 4)) || (rc = rd.wait())) return rc;
    if (timing) ms[1] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    *corres_out = corres;
    *M_out = count;
    return R3D_OK;
}

// step 3: trials in batches, compacted in t order, until maximum_tuple_count are accepted or 100 ncorr have been evaluated; one
// read-back per batch.  The rows of the accepted trials, three per trial.
int fgr_tuple_stage(r3d_ctx *ctx, DevArena &ar, const r3d_fgr_params *p, const double *rows, int64_t ncorr, double **out_rows, int64_t *trials_out,
                    int64_t *tuples_out) {
    *out_rows = nullptr; *trials_out = 0; *tuples_out = 0;
    if (ncorr == 0) return R3D_OK;
    const int64_t total = FGR_TRIALS_PER_PAIR * ncorr, maxc = std::min<int64_t>(p->maximum_tuple_count, total);
    if (maxc * 3 > 0x7fffffff) return r3d_fail(ctx, R3D_E_UNSUPPORTED, "fgr: up to %lld tuples give more than 2^31 - 1 rows", (long long)maxc);
    const int batch = (int)std::min<int64_t>(p->batch > 0 ? p->batch : RANSAC_DEFAULT_BATCH, std::min<int64_t>(RANSAC_MAX_BATCH, total));
    double *out = (double *)ar.get((size_t)maxc * 3 * 48);
    int *flags = (int *)ar.get((size_t)(batch + 1) * 4), *scan = (int *)ar.get((size_t)(batch + 1) * 4), *cut = (int *)ar.get(4);
    int *scan_part = (int *)ar.get((size_t)((batch + 1 + SCAN_TILE - 1) / SCAN_TILE) * 4);
    if (ar.rc) return ar.rc;
    int64_t have = 0, t0 = 0, trials = total;
    while (t0 < total && have < maxc) {
        const int count = (int)std::min<int64_t>(batch, total - t0);
        const unsigned nb = (unsigned)((count + 255) / 256);
        k_fgr_tuples<<<nb, 256, 0, ctx->stream>>>(rows, ncorr, p->seed, t0, count, p->tuple_scale, nullptr, flags, cut);
        R3D_HIP(ctx, hipGetLastError());
        int rc;
        if ((rc = dev_exclusive_scan<int>(ctx, ar, flags, scan, (int64_t)count + 1, nullptr, nullptr, scan_part))) return rc;
        k_fgr_tuple_compact<<<nb, 256, 0, ctx->stream>>>(rows, ncorr, p->seed, t0, count, flags, scan, have, maxc, out, cut);
        R3D_HIP(ctx, hipGetLastError());
        int acc = 0, cutv = -1;
        PinRead rd(ctx);
        if ((rc = rd.add(&acc, scan + count, 4)) || (rc = rd.add(&cutv, cut, 4)) || (rc = rd.wait())) return rc;
        if (have + acc >= maxc) {
            if (cutv < 0 || cutv >= count) return r3d_fail(ctx, R3D_E_HIP, "fgr: the tuple cut was not recorded (batch at trial %lld)", (long long)t0);
            trials = t0 + cutv + 1;
            have = maxc;
            break;
        }
        have += acc;
        t0 += count;
    }
    *out_rows = out;
    *trials_out = trials;
    *tuples_out = have;
    return R3D_OK;
}

// step 4: the loop in one launch.  trace_T / trace_par (host, optional): the state after every iteration; with fewer than
// FGR_MIN_PAIRS rows the loop does not run and they hold the start state.
int fgr_optimise_stage(r3d_ctx *ctx, DevArena &ar, const r3d_fgr_params *p, const double *rows, int64_t M, double par0, double trans[16],
                       double *final_par, double *trace_T, double *trace_par) {
    const int it = p->iteration_number;
    for (int i = 0; i < 16; i++) trans[i] = (i % 5 == 0);
    *final_par = par0;
    if (M < FGR_MIN_PAIRS || it == 0) {
        for (int k = 0; k < it && trace_T; k++) { memcpy(trace_T + (size_t)k * 16, trans, 128); trace_par[k] = par0; }
        return R3D_OK;
    }
    double *d_out = (double *)ar.get(17 * 8), *d_tr = trace_T ? (double *)ar.get((size_t)it * 17 * 8) : nullptr;
    if (ar.rc) return ar.rc;
    // QUIRK_UNSCALED_DISTANCE (tests/fgr_ref.py): par, in normalised units, is compared with the distance as the caller gave it
    k_fgr_optimize<<<1, FGR_OPT_BLOCK, 0, ctx->stream>>>(rows, M, it, par0, p->maximum_correspondence_distance, p->division_factor,
                                                         p->decrease_mu ? 1 : 0, d_out, d_tr, d_tr ? d_tr + (size_t)it * 16 : nullptr);
    R3D_HIP(ctx, hipGetLastError());
    double h[17];
    int rc;
    PinRead rd(ctx);
    if ((rc = rd.add(h, d_out, sizeof h)) || (rc = rd.wait())) return rc;
    memcpy(trans, h, 128);
    *final_par = h[16];
    if (trace_T) {
        if ((rc = r3d_download(ctx, trace_T, d_tr, (size_t)it * 16)) || (rc = r3d_download(ctx, trace_par, d_tr + (size_t)it * 16, (size_t)it))) return rc;
        R3D_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    return R3D_OK;
}

// step 5: T_ts = [R | -R mean_t + t scale_global + mean_s] maps target to source; the result is its rigid inverse
void fgr_original_scale(const double trans[16], const FgrNorm &nm, double T[16]) {
    double tt[3];
    for (int i = 0; i < 3; i++)
        tt[i] = (trans[i * 4 + 3] * nm.scale_global -
                 ((trans[i * 4] * nm.mean_t[0] + trans[i * 4 + 1] * nm.mean_t[1]) + trans[i * 4 + 2] * nm.mean_t[2])) + nm.mean_s[i];
    for (int i = 0; i < 16; i++) T[i] = (i % 5 == 0);
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) T[i * 4 + j] = trans[j * 4 + i];
        T[i * 4 + 3] = -((trans[i] * tt[0] + trans[4 + i] * tt[1]) + trans[8 + i] * tt[2]);
    }
}

// everything over device arrays: d_corres [M][2] (correspondence form) or the feature rows (feature form, d_corres null)
int fgr_core(r3d_ctx *ctx, DevArena &ar, const r3d_fgr_params *p, const double *d_src, int64_t ns, const double *d_tgt, int64_t nt,
             const int *d_corres, int64_t M, const double *d_sf, const double *d_tf, double *T4x4, r3d_fgr_stats *stats,
             std::chrono::steady_clock::time_point t_begin) {
    // R3D_FGR_TIMING=1 (tools/gpu_bench_fgr.py): the stream is drained after every stage and the stage times go to stderr
    static const bool timing = [] { const char *e = getenv("R3D_FGR_TIMING"); return e && *e == '1'; }();
    double ms[6] = {0, 0, 0, 0, 0, 0};      // matching, mutual filter, normalise + gather, tuples, optimisation, evaluation
    auto tick = std::chrono::steady_clock::now();
    auto lap = [&](int slot) -> int {
        if (!timing) return R3D_OK;
        R3D_HIP(ctx, hipStreamSynchronize(ctx->stream));
        const auto now = std::chrono::steady_clock::now();
        ms[slot] = std::chrono::duration<double, std::milli>(now - tick).count();
        tick = now;
        return R3D_OK;
    };
    int rc;
    FgrNorm nm;
    double scale_start = 1.0;
    int *corres = const_cast<int *>(d_corres);
    if (!d_corres) {
        if ((rc = fgr_mutual(ctx, ar, d_sf, ns, d_tf, nt, &corres, &M, ms, timing))) return rc;
        tick = std::chrono::steady_clock::now();
    }
    if ((rc = fgr_normalise(ctx, ar, d_src, ns, d_tgt, nt, p->use_absolute_scale != 0, nm, &scale_start))) return rc;
    double *rows = nullptr;
    if ((rc = fgr_gather(ctx, ar, d_src, ns, d_tgt, nt, corres, M, nm, &rows))) return rc;
    if ((rc = lap(2))) return rc;
    int64_t trials = 0, tuples = 0, pairs = M;
    if (p->tuple_test) {
        double *trows = nullptr;
        if ((rc = fgr_tuple_stage(ctx, ar, p, rows, M, &trows, &trials, &tuples))) return rc;
        rows = trows;
        pairs = tuples * 3;
    }
    if ((rc = lap(3))) return rc;
    const auto t_loop = std::chrono::steady_clock::now();
    double trans[16], final_par = scale_start;
    if ((rc = fgr_optimise_stage(ctx, ar, p, rows, pairs, scale_start, trans, &final_par, nullptr, nullptr))) return rc;
    if ((rc = lap(4))) return rc;
    // QUIRK_FEW_PAIRS (tests/fgr_ref.py): with fewer than FGR_MIN_PAIRS rows trans is the identity, and the result is still taken
    // back to the clouds' units: the centroid-to-centroid translation
    fgr_original_scale(trans, nm, T4x4);
    const auto t_eval = std::chrono::steady_clock::now();
    // fitness, inlier_rmse and the correspondence count: one evaluation of the registration loop at that pose, no update
    r3d_icp_params ip = {};
    ip.mode = MODE_P2P;
    ip.max_iteration = 0;
    ip.max_correspondence_distance = p->maximum_correspondence_distance;
    ip.relative_fitness = ip.relative_rmse = 1e-6;
    r3d_icp_stats ist = {};
    double Tsame[16];
    if ((rc = icp_core(ctx, ar, &ip, {.d_s = d_src, .ns = ns, .d_t = d_tgt, .nt = nt, .init4x4 = T4x4}, Tsame, &ist, t_eval))) return rc;
    if ((rc = lap(5))) return rc;
    if (stats) {
        stats->fitness = ist.fitness;
        stats->inlier_rmse = ist.inlier_rmse;
        stats->scale_global = nm.scale_global;
        stats->scale_start = scale_start;
        stats->final_par = final_par;
        stats->correspondences = ist.correspondences;
        stats->matched = M;
        stats->trials = trials;
        stats->tuples = tuples;
        stats->pairs = pairs;
        const auto t_end = std::chrono::steady_clock::now();
        stats->setup_ms = std::chrono::duration<double, std::milli>(t_loop - t_begin).count();
        stats->loop_ms = std::chrono::duration<double, std::milli>(t_end - t_loop).count();
    }
    if (timing)
        fprintf(stderr, "[r3d fgr] matching %.3f ms, mutual filter %.3f ms, normalise+gather %.3f ms, tuples %.3f ms, optimisation %.3f ms, "
                        "evaluation %.3f ms (matched %lld, trials %lld, rows %lld)\n", ms[0], ms[1], ms[2], ms[3], ms[4], ms[5], (long long)M,
                (long long)trials, (long long)pairs);
    return R3D_OK;
}

}  // namespace

extern "C" {

static int voxel_downsample_impl(r3d_ctx *ctx, const double *xyz, const double *colors, const double *normals, int64_t n, double voxel,
                                 double *out_xyz, double *out_colors, double *out_normals, int64_t *out_n, bool tensor_grid) {
    if (!ctx) return R3D_E_BADARG;
    if (!xyz || !out_xyz || !out_n || n <= 0 || !(voxel > 0)) return r3d_fail(ctx, R3D_E_BADARG, "voxel_downsample: bad argument");
    if ((colors && !out_colors) || (normals && !out_normals)) return r3d_fail(ctx, R3D_E_BADARG, "voxel_downsample: missing output array");
    R3D_HIP(ctx, hipSetDevice(ctx->device));
    DevArena ar(ctx);
    double *d_p, *d_c = nullptr, *d_n = nullptr;
    int rc;
    if ((rc = upload(ctx, ar, xyz, n * 3, &d_p)) || (rc = upload(ctx, ar, colors, n * 3, &d_c)) || (rc = upload(ctx, ar, normals, n * 3, &d_n))) return rc;
    VoxelSegs V;
    double *d_out;
    const double *ins[3] = {d_p, d_c, d_n};
    double *outs[3] = {out_xyz, out_colors, out_normals};
    for (int a = 0; a < 3; a++) {
        if (!ins[a]) continue;
        if ((rc = a == 0 ? voxel_means(ctx, ar, d_p, n, voxel, V, &d_out, tensor_grid) : voxel_attr_means(ctx, ar, V, ins[a], n, &d_out, tensor_grid))) return rc;
        if ((rc = r3d_download(ctx, outs[a], d_out, (size_t)V.nseg * 3))) return rc;
        R3D_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    *out_n = V.nseg;
    return R3D_OK;
}

int r3d_voxel_downsample(r3d_ctx *ctx, const double *xyz, const double *colors, const double *normals, int64_t n, double voxel,
                         double *out_xyz, double *out_colors, double *out_normals, int64_t *out_n) {
    R3D_ROCTX_RANGE("r3d_voxel_downsample");
    return voxel_downsample_impl(ctx, xyz, colors, normals, n, voxel, out_xyz, out_colors, out_normals, out_n, false);
}

int r3d_voxel_downsample_tensor(r3d_ctx *ctx, const double *xyz, const double *colors, const double *normals, int64_t n, double voxel,
                                double *out_xyz, double *out_colors, double *out_normals, int64_t *out_n) {
    R3D_ROCTX_RANGE("r3d_voxel_downsample_tensor");
    return voxel_downsample_impl(ctx, xyz, colors, normals, n, voxel, out_xyz, out_colors, out_normals, out_n, true);
}

int r3d_estimate_normals(r3d_ctx *ctx, const double *xyz, int64_t n, double radius, int32_t max_nn, const double *prev_normals,
                         double *normals) {
    R3D_ROCTX_RANGE("r3d_estimate_normals");
    if (!ctx) return R3D_E_BADARG;
    if (!xyz || !normals || n <= 0 || max_nn < 1) return r3d_fail(ctx, R3D_E_BADARG, "estimate_normals: bad argument");
    if (max_nn > 128) return r3d_fail(ctx, R3D_E_UNSUPPORTED, "estimate_normals: max_nn > 128 not supported");
    R3D_HIP(ctx, hipSetDevice(ctx->device));
    DevArena ar(ctx);
    double *d_p, *d_prev = nullptr, *d_n;
    int rc;
    if ((rc = upload(ctx, ar, xyz, n * 3, &d_p)) || (rc = upload(ctx, ar, prev_normals, n * 3, &d_prev))) return rc;
    if ((rc = normals_core(ctx, ar, d_p, n, radius, max_nn, d_prev, &d_n))) return rc;
    if ((rc = r3d_download(ctx, normals, d_n, (size_t)n * 3))) return rc;
    R3D_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return R3D_OK;
}

int r3d_neighbor_score(r3d_ctx *ctx, const double *xyz, int64_t n, int32_t k, double count_radius, double *score) {
    R3D_ROCTX_RANGE("r3d_neighbor_score");
    if (!ctx) return R3D_E_BADARG;
    if (!xyz || !score || n <= 0 || (count_radius <= 0 && k < 1)) return r3d_fail(ctx, R3D_E_BADARG, "neighbor_score: bad argument");
    if (k > 128) return r3d_fail(ctx, R3D_E_UNSUPPORTED, "neighbor_score: k > 128 not supported");
    R3D_HIP(ctx, hipSetDevice(ctx->device));
    DevArena ar(ctx);
    double *d_p;
    int rc;
    if ((rc = upload(ctx, ar, xyz, n * 3, &d_p))) return rc;
    Grid G;
    const int kk = (int)std::min<int64_t>(std::max(k, 1), n);
    if ((rc = grid_build(ctx, ar, d_p, n, count_radius > 0 ? count_radius : -1.0, knn_target_occ(kk), G))) return rc;
    double *d_s = (double *)ar.get((size_t)n * 8);
    if (ar.rc) return ar.rc;
    if ((rc = launch_knn(ctx, k_knn_score, G, n, kk, count_radius, d_s))) return rc;
    if ((rc = r3d_download(ctx, score, d_s, (size_t)n))) return rc;
    R3D_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return R3D_OK;
}

int r3d_reproject_disparity(r3d_ctx *ctx, const int16_t *disp, int32_t w, int32_t h, const double *Q4x4, int32_t min_valid_x16,
                            double *out_xyz, int32_t *out_pixel, int64_t *out_n) {
    R3D_ROCTX_RANGE("r3d_reproject_disparity");
    if (!ctx) return R3D_E_BADARG;
    if (!disp || !Q4x4 || !out_xyz || !out_n || w <= 0 || h <= 0) return r3d_fail(ctx, R3D_E_BADARG, "reproject_disparity: bad argument");
    R3D_HIP(ctx, hipSetDevice(ctx->device));
    DevArena ar(ctx);
    const size_t n = (size_t)w * h;
    const int16_t *d_d;
    double *d_xyz;
    int *d_pix;
    int64_t m;
    int rc;
    if ((rc = r3d_upload(ctx, ar, disp, n, &d_d))) return rc;
    if ((rc = reproject_core(ctx, ar, d_d, w, h, Q4x4, min_valid_x16, 0.0, out_pixel != nullptr, &d_xyz, &d_pix, &m))) return rc;
    *out_n = m;
    if (m == 0) return R3D_OK;
    if ((rc = r3d_download(ctx, out_xyz, d_xyz, (size_t)m * 3)) || (rc = r3d_download(ctx, out_pixel, d_pix, (size_t)m))) return rc;
    R3D_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return R3D_OK;
}

// colour request of the _color entry points: the device image the cloud is coloured from and where the colours go
struct CloudColor { const uint8_t *d_img; int32_t stride, channels, bgr; double *out; };

static int disparity_to_cloud_impl(r3d_ctx *ctx, const int16_t *d_disp, int32_t w, int32_t h, const double *Q4x4, int32_t min_valid_x16,
                                   double max_depth, const double *pose4x4, double voxel, double normal_radius, int32_t max_nn,
                                   int64_t capacity, double *out_xyz, double *out_normals, int64_t *out_n, bool device_out,
                                   const CloudColor *color = nullptr) {
    if (!ctx) return R3D_E_BADARG;
    if (!d_disp || !Q4x4 || !out_xyz || !out_n || w <= 0 || h <= 0 || capacity < 0)
        return r3d_fail(ctx, R3D_E_BADARG, "disparity_to_cloud: bad argument");
    if (max_nn > 128) return r3d_fail(ctx, R3D_E_UNSUPPORTED, "disparity_to_cloud: max_nn > 128 not supported");
    if (max_nn > 0 && !out_normals) return r3d_fail(ctx, R3D_E_BADARG, "disparity_to_cloud: normals requested without an output array");
    ColorImage img{};
    if (color) {
        if (!color->d_img) return r3d_fail(ctx, R3D_E_BADARG, "disparity_to_cloud_color: no colour image (the colourless entry points take none)");
        if (color->channels != 1 && color->channels != 3)
            return r3d_fail(ctx, R3D_E_BADARG, "disparity_to_cloud_color: %d colour channels, must be 1 or 3", (int)color->channels);
        if ((int64_t)color->stride < (int64_t)w * color->channels)
            return r3d_fail(ctx, R3D_E_BADARG, "disparity_to_cloud_color: row stride %d below %d pixels of %d bytes", (int)color->stride, (int)w, (int)color->channels);
        if (!color->out) return r3d_fail(ctx, R3D_E_BADARG, "disparity_to_cloud_color: no output array for the colours");
        img = ColorImage{color->d_img, w, color->stride, color->bgr};
    }
    R3D_HIP(ctx, hipSetDevice(ctx->device));
    DevArena ar(ctx);
    double *d_p, *d_c = nullptr;
    int *d_pix = nullptr;
    int64_t m;
    int rc;
    // depth filter off: still drop points at infinity (W = 0, e.g. disparity 0), which no voxel grid can hold
    // Host round trips of the chain (each ~25 us of idle GPU): (1) valid-pixel count + bounding box of the posed points, (2) the voxel
    // grid's segment count + its sort's fallback test, (3) the normal grid's sort -- three, was six: reprojection, pose and box are
    // enqueued over the upper bound w * h before the count is known; the voxel sort's test travels with the segment count; the
    // normal grid reuses the box (voxel means lie inside it)
    double box[6];
    if ((rc = reproject_core(ctx, ar, d_disp, w, h, Q4x4, min_valid_x16, max_depth > 0 ? max_depth : 1.0e300, color != nullptr, &d_p, &d_pix, &m, pose4x4, box))) return rc;
    *out_n = 0;
    if (m == 0) return R3D_OK;
    if (voxel > 0) {
        VoxelSegs V;
        double *d_v;
        if ((rc = voxel_means(ctx, ar, d_p, m, voxel, V, &d_v, false, nullptr, box))) return rc;
        if (color) {   // voxel colours straight from the image bytes, in the members' order (the pose does not touch colours)
            d_c = (double *)ar.get((size_t)V.nseg * 24);
            if (ar.rc) return ar.rc;
            if (color->channels == 3) rc = launch_voxel_mean_ld<double>(ctx, ar, MemberColor<3>{d_pix, img}, V.idx, V.starts, V.nseg, m, d_c);
            else rc = launch_voxel_mean_ld<double>(ctx, ar, MemberColor<1>{d_pix, img}, V.idx, V.starts, V.nseg, m, d_c);
            if (rc) return rc;
        }
        d_p = d_v;
        m = V.nseg;
    } else if (color) {
        d_c = (double *)ar.get((size_t)m * 24);
        if (ar.rc) return ar.rc;
        const unsigned nb = (unsigned)((m + 255) / 256);
        if (color->channels == 3) k_gather_colors<3><<<nb, 256, 0, ctx->stream>>>(MemberColor<3>{d_pix, img}, m, d_c);
        else k_gather_colors<1><<<nb, 256, 0, ctx->stream>>>(MemberColor<1>{d_pix, img}, m, d_c);
        R3D_HIP(ctx, hipGetLastError());
    }
    *out_n = m;
    if (m > capacity) return r3d_fail(ctx, R3D_E_BADARG, "disparity_to_cloud: %lld points, output arrays hold %lld", (long long)m, (long long)capacity);
    double *d_n = nullptr;
    if (max_nn > 0 && (rc = normals_core(ctx, ar, d_p, m, normal_radius, max_nn, nullptr, &d_n, box))) return rc;
    const hipMemcpyKind kind = device_out ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    R3D_HIP(ctx, hipMemcpyAsync(out_xyz, d_p, (size_t)m * 24, kind, ctx->stream));
    if (d_n) R3D_HIP(ctx, hipMemcpyAsync(out_normals, d_n, (size_t)m * 24, kind, ctx->stream));
    if (d_c) R3D_HIP(ctx, hipMemcpyAsync(color->out, d_c, (size_t)m * 24, kind, ctx->stream));
    // device outputs stay ordered on the context stream (the caller's next kernel or collective on that stream sees them);
    // the arena is only reused by later calls on the same stream, so no wait is needed here either
    if (!device_out) R3D_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return R3D_OK;
}

int r3d_disparity_to_cloud_dev(r3d_ctx *ctx, const int16_t *d_disp, int32_t w, int32_t h, const double *Q4x4, int32_t min_valid_x16,
                               double max_depth, const double *pose4x4, double voxel, double normal_radius, int32_t max_nn,
                               int64_t capacity, double *out_xyz, double *out_normals, int64_t *out_n) {
    R3D_ROCTX_RANGE("r3d_disparity_to_cloud_dev");
    return disparity_to_cloud_impl(ctx, d_disp, w, h, Q4x4, min_valid_x16, max_depth, pose4x4, voxel, normal_radius, max_nn, capacity,
                                   out_xyz, out_normals, out_n, false);
}

int r3d_disparity_to_cloud_resident(r3d_ctx *ctx, const int16_t *d_disp, int32_t w, int32_t h, const double *Q4x4, int32_t min_valid_x16,
                                    double max_depth, const double *pose4x4, double voxel, double normal_radius, int32_t max_nn,
                                    int64_t capacity, double *d_out_xyz, double *d_out_normals, int64_t *out_n) {
    R3D_ROCTX_RANGE("r3d_disparity_to_cloud_resident");
    return disparity_to_cloud_impl(ctx, d_disp, w, h, Q4x4, min_valid_x16, max_depth, pose4x4, voxel, normal_radius, max_nn, capacity,
                                   d_out_xyz, d_out_normals, out_n, true);
}

int r3d_disparity_to_cloud_color_dev(r3d_ctx *ctx, const int16_t *d_disp, int32_t w, int32_t h, const double *Q4x4, int32_t min_valid_x16,
                                     double max_depth, const double *pose4x4, double voxel, double normal_radius, int32_t max_nn,
                                     const uint8_t *d_color, int32_t color_stride, int32_t color_channels, int32_t color_bgr,
                                     int64_t capacity, double *out_xyz, double *out_normals, double *out_colors, int64_t *out_n) {
    R3D_ROCTX_RANGE("r3d_disparity_to_cloud_color_dev");
    const CloudColor color{d_color, color_stride, color_channels, color_bgr, out_colors};
    return disparity_to_cloud_impl(ctx, d_disp, w, h, Q4x4, min_valid_x16, max_depth, pose4x4, voxel, normal_radius, max_nn, capacity,
                                   out_xyz, out_normals, out_n, false, &color);
}

int r3d_disparity_to_cloud_color_resident(r3d_ctx *ctx, const int16_t *d_disp, int32_t w, int32_t h, const double *Q4x4, int32_t min_valid_x16,
                                          double max_depth, const double *pose4x4, double voxel, double normal_radius, int32_t max_nn,
                                          const uint8_t *d_color, int32_t color_stride, int32_t color_channels, int32_t color_bgr,
                                          int64_t capacity, double *d_out_xyz, double *d_out_normals, double *d_out_colors, int64_t *out_n) {
    R3D_ROCTX_RANGE("r3d_disparity_to_cloud_color_resident");
    const CloudColor color{d_color, color_stride, color_channels, color_bgr, d_out_colors};
    return disparity_to_cloud_impl(ctx, d_disp, w, h, Q4x4, min_valid_x16, max_depth, pose4x4, voxel, normal_radius, max_nn, capacity,
                                   d_out_xyz, d_out_normals, out_n, true, &color);
}

int r3d_align_point_clouds(r3d_ctx *ctx, const r3d_align_params *p, const double *src, const double *src_colors, int64_t ns,
                           const double *tgt, int64_t nt, const double *init4x4, double *out_xyz, double *out_colors,
                           double *out_normals, int64_t *out_n, double *T4x4, r3d_icp_stats *stats) {
    R3D_ROCTX_RANGE("r3d_align_point_clouds");
    if (!ctx) return R3D_E_BADARG;
    if (!p || !src || !tgt || !out_xyz || !out_n || !T4x4 || ns <= 0 || nt <= 0) return r3d_fail(ctx, R3D_E_BADARG, "align: bad argument");
    if (src_colors && !out_colors) return r3d_fail(ctx, R3D_E_BADARG, "align: colours given without an output array");
    const r3d_icp_params *ip = &p->icp;
    int rc;
    if ((rc = icp_mode_check(ctx, "align", ip, p->normal_max_nn > 0, true, "this mode needs normals (normal_max_nn > 0)"))) return rc;
    if (p->normal_max_nn > 128) return r3d_fail(ctx, R3D_E_UNSUPPORTED, "align: normal_max_nn > 128 not supported");
    if (p->normal_max_nn > 0 && !out_normals) return r3d_fail(ctx, R3D_E_BADARG, "align: normals requested without an output array");
    R3D_HIP(ctx, hipSetDevice(ctx->device));
    const auto t_begin = std::chrono::steady_clock::now();
    DevArena ar(ctx);
    double *d_s, *d_t, *d_c = nullptr;
    if ((rc = upload_pair(ctx, ar, src, ns, tgt, nt, &d_s, &d_t)) || (rc = upload(ctx, ar, src_colors, ns * 3, &d_c))) return rc;
    int64_t ms = ns, mt = nt;
    double tbox[6];
    const double *tgt_box = nullptr;
    if (p->voxel_size > 0) {  // pointcloud_alignment.py:22-23
        VoxelSegs V, Vt;
        double *d_sv, *d_tv;
        if ((rc = voxel_means(ctx, ar, d_s, ns, p->voxel_size, V, &d_sv))) return rc;
        if (d_c && (rc = voxel_attr_means(ctx, ar, V, d_c, ns, &d_c))) return rc;
        d_s = d_sv;
        ms = V.nseg;
        if ((rc = voxel_means(ctx, ar, d_t, nt, p->voxel_size, Vt, &d_tv, false, tbox))) return rc;
        tgt_box = tbox;   // the search grid of the down-sampled target is laid out in the box of the target's own points (as the resident model does)
        d_t = d_tv;
        mt = Vt.nseg;
    }
    double *d_sn = nullptr, *d_tn = nullptr;
    if (p->normal_max_nn > 0) {  // pointcloud_alignment.py:27-28
        if ((rc = normals_core(ctx, ar, d_s, ms, p->normal_radius, p->normal_max_nn, nullptr, &d_sn))) return rc;
        if ((rc = normals_core(ctx, ar, d_t, mt, p->normal_radius, p->normal_max_nn, nullptr, &d_tn))) return rc;
    }
    double T[16];
    const IcpInput in = {.d_s = d_s, .ns = ms, .d_sn = d_sn, .d_t = d_t, .nt = mt, .d_tn = d_tn, .init4x4 = init4x4,
                         .tgt_enclosing = tgt_box, .tgt_spacing = p->voxel_size > 0 ? p->voxel_size : 0};
    if ((rc = icp_core(ctx, ar, ip, in, T, stats, t_begin))) return rc;  // :35-39
    memcpy(T4x4, T, sizeof T);
    double *d_o, *d_on;
    if ((rc = transform_cloud(ctx, ar, T, d_s, d_sn, ms, &d_o, &d_on))) return rc;  // :42 source.transform
    if ((rc = r3d_download(ctx, out_xyz, d_o, (size_t)ms * 3)) || (rc = r3d_download(ctx, out_normals, d_on, d_on ? (size_t)ms * 3 : 0)) ||
        (rc = r3d_download(ctx, out_colors, d_c, d_c ? (size_t)ms * 3 : 0)))
        return rc;
    R3D_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *out_n = ms;
    return R3D_OK;
}

int r3d_knn_graph(r3d_ctx *ctx, const double *xyz, int64_t n, int32_t k, double radius, int32_t *nbr, double *d2) {
    R3D_ROCTX_RANGE("r3d_knn_graph");
    if (!ctx) return R3D_E_BADARG;
    if (!xyz || !nbr || n <= 0 || k < 1) return r3d_fail(ctx, R3D_E_BADARG, "knn_graph: bad argument");
    if (k > 128) return r3d_fail(ctx, R3D_E_UNSUPPORTED, "knn_graph: k > 128 not supported");
    R3D_HIP(ctx, hipSetDevice(ctx->device));
    DevArena ar(ctx);
    double *d_p;
    int rc;
    if ((rc = upload(ctx, ar, xyz, n * 3, &d_p))) return rc;
    Grid G;
    if ((rc = grid_build(ctx, ar, d_p, n, radius, knn_target_occ(k), G))) return rc;
    int *d_nb = (int *)ar.get((size_t)n * k * 4);
    double *d_d2 = d2 ? (double *)ar.get((size_t)n * k * 8) : nullptr;
    if (ar.rc) return ar.rc;
    if ((rc = launch_knn(ctx, k_knn_graph, G, n, k, radius, d_nb, d_d2))) return rc;
    if ((rc = r3d_download(ctx, nbr, d_nb, (size_t)n * k)) || (rc = r3d_download(ctx, d2, d_d2, (size_t)n * k))) return rc;
    R3D_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return R3D_OK;
}

}  // extern "C" (reopened below)

// orient_normals_consistent_tangent_plane(k)  (normal_estimation.py:21; Open3D legacy OrientNormalsConsistentTangentPlane
// [recalled], which the tensor method delegates to).  Device: the k-NN graph.  Host, inside the library (sequential by nature):
// two Kruskal spanning trees and the breadth-first sign propagation.  Edges are visited in the total order (weight, a, b).
//   with a Delaunay edge list (r3d_orient_normals_graph): Euclidean MST of those edges (weight = squared length), re-weighted
//   1 - |n_a . n_b|; plus the k-NN edges (the point itself counts as one of the k) that are NOT Delaunay edges -- the original
//   tests membership against the set of ALL Delaunay edges, not only the EMST ones, and so does this; spanning tree of that
//   graph; propagation from the point of maximum z (first on ties), whose normal is turned towards +z.
//   without one (r3d_orient_normals): k-NN edges only, every connected component rooted at its own highest point.
namespace {
struct WEdge { double w; int a, b; };
inline bool wedge_less(const WEdge &x, const WEdge &y) {
    if (x.w != y.w) return x.w < y.w;
    if (x.a != y.a) return x.a < y.a;
    return x.b < y.b;
}
// keeps the spanning-forest edges of `edges` (sorted in place); parent is the caller's disjoint-set array (reset here)
void kruskal_forest(std::vector<WEdge> &edges, std::vector<int> &parent, std::vector<WEdge> &forest) {
    std::sort(edges.begin(), edges.end(), wedge_less);
    const int64_t n = (int64_t)parent.size();
    for (int64_t i = 0; i < n; i++) parent[i] = (int)i;
    auto find = [&](int v) { while (parent[v] != v) { parent[v] = parent[parent[v]]; v = parent[v]; } return v; };
    forest.clear();
    forest.reserve(n);
    for (const WEdge &e : edges) {
        const int ra = find(e.a), rb = find(e.b);
        if (ra == rb) continue;
        parent[ra] = rb;
        forest.push_back(e);
        if ((int64_t)forest.size() == n - 1) break;
    }
}

int orient_core(r3d_ctx *ctx, const double *xyz, int64_t n, int32_t k, const int32_t *del_edges, int64_t n_del, double *normals) {
    auto dotn = [&](int a, int b) {
        return (normals[(size_t)a * 3] * normals[(size_t)b * 3] + normals[(size_t)a * 3 + 1] * normals[(size_t)b * 3 + 1]) +
               normals[(size_t)a * 3 + 2] * normals[(size_t)b * 3 + 2];
    };
    auto flip = [&](int v) { for (int a = 0; a < 3; a++) normals[(size_t)v * 3 + a] = -normals[(size_t)v * 3 + a]; };
    // the k nearest INCLUDING the point itself (KDTreeFlann::SearchKNN(points_[v0], k)), from the device
    const int kk = (int)std::min<int64_t>((int64_t)k, std::min<int64_t>(n, 128));
    std::vector<int32_t> nbr((size_t)n * kk);
    int rc = r3d_knn_graph(ctx, xyz, n, kk, -1.0, nbr.data(), nullptr);
    if (rc) return rc;
    std::vector<int> parent(n);
    std::vector<WEdge> graph, forest;
    std::vector<unsigned long long> del_keys;   // EdgeIndex = min * n + max of every Delaunay edge, sorted
    if (del_edges) {
        std::vector<WEdge> del;
        del.reserve((size_t)n_del);
        del_keys.reserve((size_t)n_del);
        for (int64_t e = 0; e < n_del; e++) {
            const int64_t u = del_edges[2 * e], v = del_edges[2 * e + 1];
            if (u < 0 || v < 0 || u >= n || v >= n) return r3d_fail(ctx, R3D_E_BADARG, "orient_normals: edge %lld names a point outside the cloud", (long long)e);
            if (u == v) continue;
            del_keys.push_back((unsigned long long)std::min(u, v) * (unsigned long long)n + (unsigned long long)std::max(u, v));
        }
        std::sort(del_keys.begin(), del_keys.end());
        del_keys.erase(std::unique(del_keys.begin(), del_keys.end()), del_keys.end());
        for (unsigned long long key : del_keys) {
            const int a = (int)(key / (unsigned long long)n), b = (int)(key % (unsigned long long)n);
            const double dx = xyz[(size_t)a * 3] - xyz[(size_t)b * 3], dy = xyz[(size_t)a * 3 + 1] - xyz[(size_t)b * 3 + 1],
                         dz = xyz[(size_t)a * 3 + 2] - xyz[(size_t)b * 3 + 2];
            del.push_back({(dx * dx + dy * dy) + dz * dz, a, b});
        }
        kruskal_forest(del, parent, forest);                                           // Euclidean minimum spanning tree
        graph.reserve(forest.size() + (size_t)n * (kk > 1 ? kk - 1 : 0));
        for (const WEdge &e : forest) graph.push_back({1.0 - std::fabs(dotn(e.a, e.b)), e.a, e.b});
    } else {
        graph.reserve((size_t)n * (kk > 1 ? kk - 1 : 0));
    }
    const size_t n_tree_edges = graph.size();
    for (int64_t i = 0; i < n; i++)
        for (int j = 0; j < kk; j++) {
            const int q = nbr[(size_t)i * kk + j];
            if (q < 0 || q == i) continue;
            const int a = (int)std::min<int64_t>(i, q), b = (int)std::max<int64_t>(i, q);
            if (del_edges && std::binary_search(del_keys.begin(), del_keys.end(), (unsigned long long)a * (unsigned long long)n + (unsigned long long)b)) continue;
            graph.push_back({0.0, a, b});
        }
    {   // an undirected k-NN edge appears once (graph_edges.insert in the original); weights after the de-duplication
        auto first = graph.begin() + (std::ptrdiff_t)n_tree_edges;
        std::sort(first, graph.end(), [](const WEdge &x, const WEdge &y) { return x.a != y.a ? x.a < y.a : x.b < y.b; });
        graph.erase(std::unique(first, graph.end(), [](const WEdge &x, const WEdge &y) { return x.a == y.a && x.b == y.b; }), graph.end());
        for (size_t e = n_tree_edges; e < graph.size(); e++) graph[e].w = 1.0 - std::fabs(dotn(graph[e].a, graph[e].b));
    }
    kruskal_forest(graph, parent, forest);
    // adjacency of the tree (CSR)
    std::vector<int> deg(n + 1, 0);
    for (const WEdge &e : forest) { deg[e.a + 1]++; deg[e.b + 1]++; }
    for (int64_t i = 0; i < n; i++) deg[i + 1] += deg[i];
    std::vector<int> adj(forest.size() * 2), fill(deg.begin(), deg.end() - 1);
    for (const WEdge &e : forest) { adj[fill[e.a]++] = e.b; adj[fill[e.b]++] = e.a; }
    // roots: the highest point of the cloud (Delaunay graph: connected), or of every component (k-NN graph only)
    std::vector<int> roots;
    if (del_edges) {
        int top = 0;
        for (int64_t i = 1; i < n; i++) if (xyz[(size_t)i * 3 + 2] > xyz[(size_t)top * 3 + 2]) top = (int)i;
        roots.push_back(top);
    } else {
        auto find = [&](int v) { while (parent[v] != v) v = parent[v]; return v; };
        std::vector<int> comp_root(n, -1);
        for (int64_t i = 0; i < n; i++) {
            const int r = find((int)i);
            if (comp_root[r] < 0 || xyz[(size_t)i * 3 + 2] > xyz[(size_t)comp_root[r] * 3 + 2]) comp_root[r] = (int)i;
        }
        for (int64_t r = 0; r < n; r++) if (comp_root[r] >= 0) roots.push_back(comp_root[r]);
    }
    std::vector<char> seen(n, 0);
    std::vector<int> queue;
    queue.reserve(n);
    for (const int root : roots) {
        if (normals[(size_t)root * 3 + 2] < 0) flip(root);      // TestAndOrientNormal((0,0,1), n_root)
        queue.clear();
        queue.push_back(root);
        seen[root] = 1;
        for (size_t h = 0; h < queue.size(); h++) {
            const int v = queue[h];
            for (int e = deg[v]; e < deg[v + 1]; e++) {
                const int u = adj[e];
                if (seen[u]) continue;
                seen[u] = 1;
                if (dotn(u, v) < 0) flip(u);
                queue.push_back(u);
            }
        }
    }
    return R3D_OK;
}
}  // namespace

extern "C" {

int r3d_orient_normals(r3d_ctx *ctx, const double *xyz, int64_t n, int32_t k, double *normals) {
    R3D_ROCTX_RANGE("r3d_orient_normals");
    if (!ctx) return R3D_E_BADARG;
    if (!xyz || !normals || n <= 0 || k < 1) return r3d_fail(ctx, R3D_E_BADARG, "orient_normals: bad argument");
    if (n == 1) { if (normals[2] < 0) for (int a = 0; a < 3; a++) normals[a] = -normals[a]; return R3D_OK; }
    return orient_core(ctx, xyz, n, k, nullptr, 0, normals);
}

int r3d_orient_normals_graph(r3d_ctx *ctx, const double *xyz, int64_t n, int32_t k, const int32_t *delaunay_edges, int64_t n_edges,
                             double *normals) {
    R3D_ROCTX_RANGE("r3d_orient_normals_graph");
    if (!ctx) return R3D_E_BADARG;
    if (!xyz || !normals || !delaunay_edges || n <= 0 || k < 1 || n_edges < 0) return r3d_fail(ctx, R3D_E_BADARG, "orient_normals_graph: bad argument");
    if (n < 4) return r3d_fail(ctx, R3D_E_BADARG, "orient_normals_graph: a tetrahedralisation needs at least 4 points");
    return orient_core(ctx, xyz, n, k, delaunay_edges, n_edges, normals);
}

int r3d_transform_points(r3d_ctx *ctx, const double *xyz, int64_t n, const double *T4x4, int32_t rotate_only, double *out) {
    R3D_ROCTX_RANGE("r3d_transform_points");
    if (!ctx) return R3D_E_BADARG;
    if (!xyz || !out || !T4x4 || n <= 0) return r3d_fail(ctx, R3D_E_BADARG, "transform_points: bad argument");
    R3D_HIP(ctx, hipSetDevice(ctx->device));
    DevArena ar(ctx);
    double *d_p;
    int rc;
    if ((rc = upload(ctx, ar, xyz, n * 3, &d_p))) return rc;
    double *d_o = (double *)ar.get((size_t)n * 24);
    if (ar.rc) return ar.rc;
    k_transform<<<(unsigned)((n + 255) / 256), 256, 0, ctx->stream>>>(d_p, n, to_rigid(T4x4), rotate_only, d_o);
    R3D_HIP(ctx, hipGetLastError());
    if ((rc = r3d_download(ctx, out, d_o, (size_t)n * 3))) return rc;
    R3D_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return R3D_OK;
}

int r3d_icp(r3d_ctx *ctx, const r3d_icp_params *p, const double *src, int64_t ns, const double *src_normals, const double *tgt,
            int64_t nt, const double *tgt_normals, const double *init4x4, double *T4x4, r3d_icp_stats *stats) {
    R3D_ROCTX_RANGE("r3d_icp");
    if (!ctx) return R3D_E_BADARG;
    if (!p || !src || !tgt || !T4x4 || ns <= 0 || nt <= 0) return r3d_fail(ctx, R3D_E_BADARG, "icp: bad argument");
    int rc;
    if ((rc = icp_mode_check(ctx, "icp", p, tgt_normals != nullptr, src_normals != nullptr))) return rc;
    R3D_HIP(ctx, hipSetDevice(ctx->device));
    const auto t_begin = std::chrono::steady_clock::now();
    DevArena ar(ctx);
    double *d_t, *d_tn = nullptr, *d_s, *d_sn = nullptr;
    if ((rc = upload_pair(ctx, ar, src, ns, tgt, nt, &d_s, &d_t)) || (rc = upload(ctx, ar, src_normals, ns * 3, &d_sn)) ||
        (rc = upload(ctx, ar, tgt_normals, nt * 3, &d_tn)))
        return rc;
    return icp_core(ctx, ar, p, {.d_s = d_s, .ns = ns, .d_sn = d_sn, .d_t = d_t, .nt = nt, .d_tn = d_tn, .init4x4 = init4x4}, T4x4, stats, t_begin);
}

// ---- resident scan-loop model (main.py:34-54, test/GICP1.py:134-155) ---------------------------------
// The reference keeps the growing model in an Open3D cloud and hands ALL of it to align_point_clouds for every frame, which
// voxel-down-samples it again (pointcloud_alignment.py:22-23).  Here the model's points / colours / normals live in device
// buffers owned by an r3d_model: a frame goes up, the 4x4 and the statistics come down, nothing else crosses PCIe until
// r3d_model_download.  Every step runs the same kernels in the same order as the one-shot entry points on the same values
// (the model is re-voxelised from its resident points, in their original order), so the results are identical to them.
}  // extern "C"
namespace {
// the device arrays of a voxel table, one entry per voxel in key order; all null when there is no table
struct VtView { const unsigned long long *keys = nullptr; const double *sums = nullptr; const int *cnt = nullptr; };
// Incremental legacy voxel table of the model's points (k_vt_*), double-buffered for the merge.  The one invariant: `valid` implies
// that the buffers at `cur` hold exactly the table of the model rows [0, rows) for voxel size `voxel` and minimum corner `min`: n
// voxels, the rows' maximum corner in `max`.  table_rebuild and table_update keep it by dropping `valid` before they write into a
// resident buffer and setting it again, with the fields that describe the table, after their last step that can fail: whatever
// stops them in between, the next call finds no table and rebuilds.
struct VoxelTable {
    bool valid = false;
    double voxel = 0, min[3] = {0, 0, 0}, max[3] = {0, 0, 0};
    int64_t n = 0, rows = 0;
    r3d_buf keys[2], sums[2], cnt[2];
    int cur = 0;
    int rebuilds = 0, updates = 0;   // successful ones (r3d_model_voxel_table_stats)
    int fail_step = 0;               // r3d_model_debug_fail_table_step: armed for the next model_target_voxels only

    struct Set { unsigned long long *keys; double *sums; int *cnt; };
    Set set(int i) const { return {(unsigned long long *)keys[i].p, (double *)sums[i].p, (int *)cnt[i].p}; }
    Set current() const { return set(cur); }
    Set other() const { return set(cur ^ 1); }
    VtView view() const { return valid ? VtView{current().keys, current().sums, current().cnt} : VtView(); }
    // no table; the buffers and the statistics stay
    void invalidate() { valid = false; n = rows = 0; }
    // grow-only room for `voxels` entries in buffer set i; the policy frees before it allocates, so a failure leaves null buffers
    int reserve(r3d_ctx *ctx, int i, int64_t voxels) {
        int rc;
        if ((rc = keys[i].reserve(ctx, ctx->stream, (size_t)voxels * 8, R3D_GROW_VOXEL_TABLE))) return rc;
        if ((rc = sums[i].reserve(ctx, ctx->stream, (size_t)voxels * 24, R3D_GROW_VOXEL_TABLE))) return rc;
        return cnt[i].reserve(ctx, ctx->stream, (size_t)voxels * 4, R3D_GROW_VOXEL_TABLE);
    }
};
// Bounding box of the rows [lo, hi) the last alignment appended: computed on the device when they were appended, fetched with the
// NEXT call's first read-back (no round trip of its own); host_ok: `box` holds it already
struct PendingBox {
    r3d_buf dev;
    int64_t lo = 0, hi = 0;
    bool host_ok = false;
    double box[6] = {0, 0, 0, 0, 0, 0};

    bool covers(int64_t a, int64_t b) const { return host_ok && lo == a && hi == b; }
    void reset() { lo = hi = 0; host_ok = false; }
    void set(int64_t a, int64_t b) { lo = a; hi = b; }   // the box of rows [a, b) has been enqueued into `dev`
    // the read-back that brings an enqueued box to `box`; empty when there is none or the host has it (the caller sets host_ok
    // once the read has come through)
    PinExtra fetch() {
        PinExtra e;
        if (dev.p && hi > lo && !host_ok) { e.host = box; e.dev = dev.p; e.bytes = 48; }
        return e;
    }
};
}  // namespace
struct r3d_model {
    r3d_ctx *ctx = nullptr;
    r3d_buf pts, cols, nrms;
    int64_t n = 0;
    bool has_colors = false, has_normals = false;
    VoxelTable table;
    PendingBox pend;
};
namespace {
// grows a model buffer to hold `rows` triplets, keeping the first `keep` rows
int model_rows(r3d_model *m, r3d_buf &b, int64_t rows, int64_t keep) {
    return b.reserve(m->ctx, m->ctx->stream, (size_t)rows * 24, R3D_GROW_MODEL, keep > 0 ? (size_t)keep * 24 : 0);
}
// appends n rows (device or host source) with the attribute rule of the legacy operator+= (an attribute survives only when
// the model is empty or already carries it AND the appended cloud carries it)
int model_append(r3d_model *m, const double *xyz, const double *colors, const double *normals, int64_t n, hipMemcpyKind kind) {
    r3d_ctx *ctx = m->ctx;
    const bool keep_c = (m->n == 0 || m->has_colors) && colors, keep_n = (m->n == 0 || m->has_normals) && normals;
    int rc;
    if ((rc = model_rows(m, m->pts, m->n + n, m->n))) return rc;
    if (keep_c && (rc = model_rows(m, m->cols, m->n + n, m->n))) return rc;
    if (keep_n && (rc = model_rows(m, m->nrms, m->n + n, m->n))) return rc;
    R3D_HIP(ctx, hipMemcpyAsync((double *)m->pts.p + m->n * 3, xyz, (size_t)n * 24, kind, ctx->stream));
    if (keep_c) R3D_HIP(ctx, hipMemcpyAsync((double *)m->cols.p + m->n * 3, colors, (size_t)n * 24, kind, ctx->stream));
    if (keep_n) R3D_HIP(ctx, hipMemcpyAsync((double *)m->nrms.p + m->n * 3, normals, (size_t)n * 24, kind, ctx->stream));
    if (kind == hipMemcpyHostToDevice) R3D_HIP(ctx, hipStreamSynchronize(ctx->stream));   // the caller may reuse its arrays
    m->has_colors = keep_c;
    m->has_normals = keep_n;
    m->n += n;
    return R3D_OK;
}
}  // namespace
extern "C" {

int r3d_model_create(r3d_ctx *ctx, r3d_model **out) {
    if (!ctx || !out) return R3D_E_BADARG;
    r3d_model *m = new (std::nothrow) r3d_model;
    if (!m) return r3d_fail(ctx, R3D_E_OOM, "model_create: out of host memory");
    m->ctx = ctx;
    *out = m;
    return R3D_OK;
}

void r3d_model_destroy(r3d_model *m) {
    if (!m) return;
    (void)hipSetDevice(m->ctx->device);
    (void)hipStreamSynchronize(m->ctx->stream);
    delete m;
}

int r3d_model_clear(r3d_model *m) {
    if (!m) return R3D_E_BADARG;
    m->n = 0;
    m->has_colors = m->has_normals = false;
    m->table.invalidate();
    m->pend.reset();
    return R3D_OK;
}

int r3d_model_size(r3d_model *m, int64_t *n, int32_t *has_colors, int32_t *has_normals) {
    if (!m) return R3D_E_BADARG;
    if (n) *n = m->n;
    if (has_colors) *has_colors = m->has_colors;
    if (has_normals) *has_normals = m->has_normals;
    return R3D_OK;
}

int r3d_model_voxel_table_stats(r3d_model *m, int64_t *voxels, int32_t *rebuilds, int32_t *updates) {
    if (!m) return R3D_E_BADARG;
    if (voxels) *voxels = m->table.n;   // 0 without a table (VoxelTable::invalidate)
    if (rebuilds) *rebuilds = m->table.rebuilds;
    if (updates) *updates = m->table.updates;
    return R3D_OK;
}

int r3d_model_debug_fail_table_step(r3d_model *m, int32_t step) {
    if (!m) return R3D_E_BADARG;
    if (step < 0 || step > 3) return r3d_fail(m->ctx, R3D_E_BADARG, "model_debug_fail_table_step: step must be 0..3");
    m->table.fail_step = step;
    return R3D_OK;
}

int r3d_model_append(r3d_model *m, const double *xyz, const double *colors, const double *normals, int64_t n) {
    R3D_ROCTX_RANGE("r3d_model_append");
    if (!m) return R3D_E_BADARG;
    r3d_ctx *ctx = m->ctx;
    if (!xyz || n < 0) return r3d_fail(ctx, R3D_E_BADARG, "model_append: bad argument");
    if (n == 0) return R3D_OK;
    R3D_HIP(ctx, hipSetDevice(ctx->device));
    return model_append(m, xyz, colors, normals, n, hipMemcpyHostToDevice);
}

}  // extern "C"
namespace {
// The key space of the table: fewer than 2^21 voxels along every axis, counted from the grid's origin (the minimum corner less
// half a voxel)
bool vt_key_space_ok(const double *mn, const double *mx, double voxel) {
    for (int a = 0; a < 3; a++) if (!((mx[a] - (mn[a] - 0.5 * voxel)) / voxel < 2097000.0)) return false;
    return true;
}
// r3d_model_debug_fail_table_step: the error return that was asked for at point `step` of this call; nothing else happens there
int table_injected(r3d_ctx *ctx, int armed, int step) {
    return armed == step ? r3d_fail(ctx, R3D_E_HIP, "model voxel table: injected failure at step %d", step) : R3D_OK;
}
// What a call does about the table.  R3D_MODEL_IMPL=rebuild: no table, the full sort of every model point, every frame.
enum TableStep { TABLE_FULL_PASS, TABLE_REBUILD, TABLE_UPDATE, TABLE_KEEP };
// Decides and changes nothing.  Rebuild: there is no table for this voxel size, or the slice of rows the table does not cover yet
// lies below the table's minimum corner (the grid origin moves: every key changes), or it reaches beyond the key space (the rebuild
// then finds the same and ends in the plain full pass).  Update: nmx receives the maximum corner of the table's rows and the
// slice.  The slice's box is the pending box when the slice is the block the last alignment appended, a pass over it otherwise.
int table_decide(const r3d_model *m, DevArena &ar, double voxel, TableStep *step, double nmx[3]) {
    static const bool always_rebuild = [] { const char *e = getenv("R3D_MODEL_IMPL"); return e && !strcmp(e, "rebuild"); }();
    r3d_ctx *ctx = m->ctx;
    const VoxelTable &t = m->table;
    *step = always_rebuild ? TABLE_FULL_PASS : TABLE_REBUILD;
    if (always_rebuild || !t.valid || t.voxel != voxel || t.rows > m->n) return R3D_OK;
    if (t.rows == m->n) { *step = TABLE_KEEP; return R3D_OK; }
    int rc;
    double smn[3], smx[3];
    if (m->pend.covers(t.rows, m->n)) {
        for (int a = 0; a < 3; a++) { smn[a] = m->pend.box[a]; smx[a] = m->pend.box[3 + a]; }
        if ((rc = bbox_check(ctx, smn, smx))) return rc;
    } else if ((rc = cloud_bbox(ctx, ar, (const double *)m->pts.p + t.rows * 3, m->n - t.rows, smn, smx))) return rc;
    for (int a = 0; a < 3; a++) {
        if (smn[a] < t.min[a]) return R3D_OK;
        nmx[a] = std::max(t.max[a], smx[a]);
    }
    if (vt_key_space_ok(t.min, nmx, voxel)) *step = TABLE_UPDATE;
    return R3D_OK;
}
// The plain full pass, as the one-shot entry points make it: no table is read or written.  known_bounds: the model's box when
// the caller has it
int model_full_pass(r3d_model *m, DevArena &ar, double voxel, const double *known_bounds, double **d_tv_out, int64_t *mt_out, double *box_out) {
    VoxelSegs Vt;
    if (known_bounds) for (int a = 0; a < 6; a++) box_out[a] = known_bounds[a];
    if (int rc = voxel_means(m->ctx, ar, (const double *)m->pts.p, m->n, voxel, Vt, d_tv_out, false, known_bounds ? nullptr : box_out, known_bounds)) return rc;
    *mt_out = Vt.nseg;
    return R3D_OK;
}
// The table of all model rows, built from nothing into the buffers at `cur`.  bounds receives the model's box.  More than 2^21
// voxels along an axis: success without a table (the caller makes the plain full pass).  An error return leaves no table either.
int table_rebuild(r3d_model *m, DevArena &ar, double voxel, int fail, double bounds[6]) {
    r3d_ctx *ctx = m->ctx;
    VoxelTable &t = m->table;
    const double *d_t = (const double *)m->pts.p;
    int rc;
    if ((rc = cloud_bbox(ctx, ar, d_t, m->n, bounds, bounds + 3))) return rc;   // (the pass voxel_segments would make itself)
    if (!vt_key_space_ok(bounds, bounds + 3, voxel)) {
        t.invalidate();
        return R3D_OK;
    }
    VoxelSegs Vt;
    if ((rc = voxel_segments(ctx, ar, d_t, m->n, voxel, Vt, false, nullptr, nullptr, nullptr, bounds))) return rc;
    t.invalidate();   // the reserve may free the buffers at `cur` and the build overwrites them
    if ((rc = t.reserve(ctx, t.cur, Vt.nseg))) return rc;
    const VoxelTable::Set c = t.current();
    k_vt_build<8><<<(unsigned)((Vt.nseg + 255) / 256), 256, 0, ctx->stream>>>(Vt.sorted, Vt.starts, Vt.nseg, m->n, bounds[0] - 0.5 * voxel,
                                                                           bounds[1] - 0.5 * voxel, bounds[2] - 0.5 * voxel, voxel, c.keys, c.sums, c.cnt);
    R3D_HIP(ctx, hipGetLastError());
    if ((rc = table_injected(ctx, fail, 1))) return rc;
    for (int a = 0; a < 3; a++) { t.min[a] = bounds[a]; t.max[a] = bounds[3 + a]; }
    t.voxel = voxel;
    t.n = Vt.nseg;
    t.rows = m->n;
    t.valid = true;
    t.rebuilds++;
    return R3D_OK;
}
// The rows the table does not cover yet, [rows, m->n), merged into it: their runs are added to the sums of the voxels that exist,
// in place, and the voxels they open are merged into the other buffer set, which then becomes `cur`.  nmx: table_decide's.
// Up to and including the reserve of the other buffers nothing resident is touched and an error return keeps the table.  From
// k_vt_update on the sums at `cur` hold part of the slice, so the table is marked invalid before that launch and valid again only
// after the last step that can fail.  The table is not made transactional by copying it first: an update that fails in between
// costs one full rebuild on the next call.
int table_update(r3d_model *m, DevArena &ar, double voxel, const double nmx[3], int fail) {
    r3d_ctx *ctx = m->ctx;
    VoxelTable &t = m->table;
    int rc;
    const int64_t ns = m->n - t.rows, tn = t.n;
    double org[3];
    for (int a = 0; a < 3; a++) org[a] = t.min[a] - 0.5 * voxel;
    VoxelSegs V;
    if ((rc = voxel_segments(ctx, ar, (const double *)m->pts.p + t.rows * 3, ns, voxel, V, false, org, nmx))) return rc;
    if ((rc = t.reserve(ctx, t.cur ^ 1, tn + V.nseg))) return rc;
    unsigned long long *segkey = (unsigned long long *)ar.get((size_t)V.nseg * 8);
    int64_t *ins = (int64_t *)ar.get((size_t)V.nseg * 8);
    double *nsum = (double *)ar.get((size_t)V.nseg * 24);
    int *is_new = (int *)ar.get((size_t)V.nseg * 4), *rank = (int *)ar.get((size_t)V.nseg * 4), *ncnt = (int *)ar.get((size_t)V.nseg * 4);
    if (ar.rc) return ar.rc;
    const VoxelTable::Set c = t.current(), o = t.other();
    const unsigned nbs = (unsigned)((V.nseg + 255) / 256);
    t.invalidate();
    k_vt_update<<<nbs, 256, 0, ctx->stream>>>(V.sorted, V.starts, V.nseg, ns, org[0], org[1], org[2], voxel, c.keys, tn, c.sums, c.cnt, segkey, is_new,
                                              ins, nsum, ncnt);
    if ((rc = table_injected(ctx, fail, 2))) return rc;
    if (int src = dev_exclusive_scan<int>(ctx, ar, is_new, rank, V.nseg)) return src;
    CompactCount cc(rank, is_new, V.nseg);
    PinRead rd(ctx);
    if ((rc = cc.add_to(rd)) || (rc = rd.wait())) return rc;
    const int total_new = (int)cc.count();
    if (total_new > 0) {
        k_vt_merge<<<(unsigned)((tn + V.nseg + 255) / 256), 256, 0, ctx->stream>>>(c.keys, c.sums, c.cnt, tn, segkey, is_new, rank, ins, nsum, ncnt, V.nseg,
                                                                                  total_new, o.keys, o.sums, o.cnt);
        if ((rc = table_injected(ctx, fail, 3))) return rc;
    }
    R3D_HIP(ctx, hipGetLastError());
    if (total_new > 0) t.cur ^= 1;   // the merged table is in the other buffers; without a new voxel the sums went on in place
    t.n = tn + total_new;
    for (int a = 0; a < 3; a++) t.max[a] = nmx[a];
    t.rows = m->n;
    t.valid = true;
    t.updates++;
    return R3D_OK;
}
// The means of the table's voxels in a fresh arena buffer, the model's box, and the table's arrays for the diagnostic read-out
int table_emit(r3d_model *m, DevArena &ar, double **d_tv_out, int64_t *mt_out, double *box_out, VtView *table_out) {
    r3d_ctx *ctx = m->ctx;
    const VoxelTable &t = m->table;
    if (table_out) *table_out = t.view();
    double *d_tv = (double *)ar.get((size_t)t.n * 24);
    if (ar.rc) return ar.rc;
    k_vt_means<<<(unsigned)((t.n + 255) / 256), 256, 0, ctx->stream>>>(t.current().sums, t.current().cnt, t.n, d_tv);
    R3D_HIP(ctx, hipGetLastError());
    for (int a = 0; a < 3; a++) { box_out[a] = t.min[a]; box_out[3 + a] = t.max[a]; }
    *d_tv_out = d_tv;
    *mt_out = t.n;
    return R3D_OK;
}
// pointcloud_alignment.py:23 for the resident model: the legacy voxel grid of ALL model points, as means in lexicographic voxel
// order in a fresh arena buffer.  Default: the incremental table (full rebuild whenever the model's minimum corner moved, the
// voxel size changed or the table does not exist); R3D_MODEL_IMPL=rebuild: the full sort of every model point, every frame.
// table_out (r3d_model_debug_voxel_table): the resident table's device arrays behind the means, all null when there is none
int model_target_voxels(r3d_model *m, DevArena &ar, double voxel, double **d_tv_out, int64_t *mt_out, double *box_out /* [6]: the model's box */,
                        VtView *table_out = nullptr) {
    const int fail = std::exchange(m->table.fail_step, 0);   // one shot: armed for this call only, whether or not it gets there
    if (table_out) *table_out = VtView();
    int rc;
    TableStep step;
    double nmx[3], bounds[6];
    if ((rc = table_decide(m, ar, voxel, &step, nmx))) return rc;
    if (step == TABLE_FULL_PASS) return model_full_pass(m, ar, voxel, nullptr, d_tv_out, mt_out, box_out);
    if (step == TABLE_REBUILD) {
        if ((rc = table_rebuild(m, ar, voxel, fail, bounds))) return rc;
        if (!m->table.valid) return model_full_pass(m, ar, voxel, bounds, d_tv_out, mt_out, box_out);   // beyond the key space: no table
    } else if (step == TABLE_UPDATE && (rc = table_update(m, ar, voxel, nmx, fail))) return rc;
    return table_emit(m, ar, d_tv_out, mt_out, box_out, table_out);
}
int model_align_checks(r3d_model *m, const r3d_align_params *p, const char *who) {
    r3d_ctx *ctx = m->ctx;
    if (m->n <= 0) return r3d_fail(ctx, R3D_E_BADARG, "%s: the model is empty (append the first frame)", who);
    if (int rc = icp_mode_check(ctx, who, &p->icp, p->normal_max_nn > 0, true, "this mode needs normals (normal_max_nn > 0)")) return rc;
    if (p->normal_max_nn > 128) return r3d_fail(ctx, R3D_E_UNSUPPORTED, "%s: normal_max_nn > 128 not supported", who);
    return R3D_OK;
}
// the frame (d_s, optional colours d_c, ns points) is already on the device in arena `ar`
int model_align_core(r3d_model *m, DevArena &ar, const r3d_align_params *p, double *d_s, double *d_c, int64_t ns, double *T4x4,
                     r3d_icp_stats *stats, int64_t *appended, std::chrono::steady_clock::time_point t_begin,
                     const double *frame_box = nullptr /* bounding box of the frame's points when the caller already has it */) {
    r3d_ctx *ctx = m->ctx;
    const r3d_icp_params *ip = &p->icp;
    int rc;
    double *d_t = (double *)m->pts.p;
    int64_t ms = ns, mt = m->n;
    const double *tgt_box = nullptr;
    double tbox[6];
    if (p->voxel_size > 0) {  // pointcloud_alignment.py:22-23 on the frame and on the WHOLE resident model
        VoxelSegs V;
        double *d_sv;
        if ((rc = voxel_means(ctx, ar, d_s, ns, p->voxel_size, V, &d_sv, false, nullptr, frame_box))) return rc;
        if (d_c && (rc = voxel_attr_means(ctx, ar, V, d_c, ns, &d_c))) return rc;
        d_s = d_sv;
        ms = V.nseg;
        double *d_tv = nullptr;
        if ((rc = model_target_voxels(m, ar, p->voxel_size, &d_tv, &mt, tbox))) return rc;
        d_t = d_tv;
        tgt_box = tbox;   // the model's own box (the table keeps it): the voxel means lie inside it, no bounding-box pass for the search grid
    }
    // pointcloud_alignment.py:27-28 estimates normals on both clouds.  The point-to-point estimator never reads them and the
    // model's operator+= drops the frame's normals unless the model carries normals itself, so they are computed only where
    // they can reach a result: target normals for the plane / GICP estimators, source normals for GICP or a model with normals.
    double *d_sn = nullptr, *d_tn = nullptr;
    const bool want_sn = p->normal_max_nn > 0 && (ip->mode == MODE_GICP || m->has_normals);
    if (want_sn && (rc = normals_core(ctx, ar, d_s, ms, p->normal_radius, p->normal_max_nn, nullptr, &d_sn))) return rc;
    if (ip->mode != MODE_P2P && (rc = normals_core(ctx, ar, d_t, mt, p->normal_radius, p->normal_max_nn, nullptr, &d_tn))) return rc;
    double T[16];
    const IcpInput in = {.d_s = d_s, .ns = ms, .d_sn = d_sn, .d_t = d_t, .nt = mt, .d_tn = d_tn,
                         .tgt_enclosing = tgt_box, .tgt_spacing = p->voxel_size > 0 ? p->voxel_size : 0};
    if ((rc = icp_core(ctx, ar, ip, in, T, stats, t_begin))) return rc;  // :35-39, from identity
    memcpy(T4x4, T, sizeof T);
    double *d_o, *d_on;
    if ((rc = transform_cloud(ctx, ar, T, d_s, d_sn, ms, &d_o, &d_on))) return rc;  // :42 source.transform
    const int64_t n_before = m->n;
    if ((rc = model_append(m, d_o, d_c, d_on, ms, hipMemcpyDeviceToDevice))) return rc;   // main.py:49 combined += aligned
    if (appended) *appended = ms;
    // the appended block's bounding box, for the next frame's table update: enqueued now, fetched with that call's first read-back
    m->pend.reset();
    if (p->voxel_size > 0 && ms > 0) {
        if (!m->pend.dev.p && m->pend.dev.alloc(64) != hipSuccess) return R3D_OK;   // no pending box: the next call computes it itself
        if (cloud_bbox_enqueue_dn(ctx, ar, d_o, ms, nullptr, nullptr, nullptr, (double *)m->pend.dev.p) == R3D_OK) m->pend.set(n_before, m->n);
    }
    return R3D_OK;
}
}  // namespace
extern "C" {

int r3d_model_align_append(r3d_model *m, const r3d_align_params *p, const double *src, const double *src_colors, int64_t ns,
                           double *T4x4, r3d_icp_stats *stats, int64_t *appended) {
    R3D_ROCTX_RANGE("r3d_model_align_append");
    if (!m) return R3D_E_BADARG;
    r3d_ctx *ctx = m->ctx;
    if (!p || !src || !T4x4 || ns <= 0) return r3d_fail(ctx, R3D_E_BADARG, "model_align_append: bad argument");
    int rc;
    if ((rc = model_align_checks(m, p, "model_align_append"))) return rc;
    R3D_HIP(ctx, hipSetDevice(ctx->device));
    const auto t_begin = std::chrono::steady_clock::now();
    DevArena ar(ctx);
    double *d_s, *d_c = nullptr;
    if ((rc = upload(ctx, ar, src, ns * 3, &d_s)) || (rc = upload(ctx, ar, src_colors, ns * 3, &d_c))) return rc;
    return model_align_core(m, ar, p, d_s, d_c, ns, T4x4, stats, appended, t_begin);
}

// diagnostic: the model's voxel grid as the next r3d_model_align_append with this voxel size would see it -- the same
// model_target_voxels call (the table is brought up to date with every model row, the statistics advance), then the table read out
// entry by entry (tests/test_voxel_edges_gpu.py compares it with tests/voxel_ref.py)
int r3d_model_debug_voxel_table(r3d_model *m, double voxel, int64_t cap, uint64_t *keys, double *sums, int32_t *counts, double *means,
                                double *box6, int64_t *n_out, int32_t *resident) {
    R3D_ROCTX_RANGE("r3d_model_debug_voxel_table");
    if (!m) return R3D_E_BADARG;
    r3d_ctx *ctx = m->ctx;
    if (m->n <= 0) return r3d_fail(ctx, R3D_E_BADARG, "model_debug_voxel_table: the model is empty");
    if (!(voxel > 0)) return r3d_fail(ctx, R3D_E_BADARG, "model_debug_voxel_table: voxel must be > 0");
    R3D_HIP(ctx, hipSetDevice(ctx->device));
    DevArena ar(ctx);
    int rc;
    double *d_tv = nullptr, box[6];
    int64_t n = 0;
    VtView vt;
    if ((rc = model_target_voxels(m, ar, voxel, &d_tv, &n, box, &vt))) return rc;
    if (n_out) *n_out = n;
    if (resident) *resident = vt.keys != nullptr;
    if (n <= cap) {
        if (box6) memcpy(box6, box, sizeof box);
        if ((rc = r3d_download(ctx, means, d_tv, (size_t)n * 3))) return rc;
        if (vt.keys && ((rc = r3d_download(ctx, keys, (const uint64_t *)vt.keys, (size_t)n)) || (rc = r3d_download(ctx, sums, vt.sums, (size_t)n * 3)) ||
                        (rc = r3d_download(ctx, counts, vt.cnt, (size_t)n))))
            return rc;
    }
    R3D_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return R3D_OK;
}

// The same two steps of main.py:34-49 for a frame that is still a DEPTH IMAGE (the recorded frames of test/output84, a RealSense
// z16 frame): create_from_rgbd_image + flip (test/check84.py:155-159,172-178) runs on the device, so a 0.6 MB image goes up
// instead of 6.8 MB of float64 points.  color (may be NULL): uint8 [h][w][3], channels taken in the order given.
int r3d_model_append_depth(r3d_model *m, const uint16_t *depth, int32_t w, int32_t h, int32_t stride, const r3d_depth_camera *cam,
                           const uint8_t *color, int32_t color_stride, int64_t *appended) {
    R3D_ROCTX_RANGE("r3d_model_append_depth");
    if (!m) return R3D_E_BADARG;
    r3d_ctx *ctx = m->ctx;
    int rc;
    if ((rc = depth_args_ok(ctx, depth, w, h, stride, cam, color, color_stride, "model_append_depth"))) return rc;
    R3D_HIP(ctx, hipSetDevice(ctx->device));
    DevArena ar(ctx);
    double *d_p, *d_c;
    int64_t n;
    if ((rc = backproject_core(ctx, ar, depth, w, h, stride, cam, color, color_stride, false, &d_p, &d_c, nullptr, &n))) return rc;
    if (appended) *appended = n;
    if (n == 0) return R3D_OK;
    return model_append(m, d_p, d_c, nullptr, n, hipMemcpyDeviceToDevice);
}

int r3d_model_align_append_depth(r3d_model *m, const r3d_align_params *p, const uint16_t *depth, int32_t w, int32_t h, int32_t stride,
                                 const r3d_depth_camera *cam, const uint8_t *color, int32_t color_stride, double *T4x4, r3d_icp_stats *stats,
                                 int64_t *frame_points, int64_t *appended) {
    R3D_ROCTX_RANGE("r3d_model_align_append_depth");
    if (!m) return R3D_E_BADARG;
    r3d_ctx *ctx = m->ctx;
    if (!p || !T4x4) return r3d_fail(ctx, R3D_E_BADARG, "model_align_append_depth: bad argument");
    int rc;
    if ((rc = depth_args_ok(ctx, depth, w, h, stride, cam, color, color_stride, "model_align_append_depth"))) return rc;
    if ((rc = model_align_checks(m, p, "model_align_append_depth"))) return rc;
    R3D_HIP(ctx, hipSetDevice(ctx->device));
    const auto t_begin = std::chrono::steady_clock::now();
    DevArena ar(ctx);
    double *d_p, *d_c;
    int64_t n;
    double fbox[6];
    PinExtra pend = m->pend.fetch();
    if ((rc = backproject_core(ctx, ar, depth, w, h, stride, cam, color, color_stride, false, &d_p, &d_c, nullptr, &n, fbox, &pend))) return rc;
    if (pend.host) m->pend.host_ok = true;
    if (frame_points) *frame_points = n;
    if (appended) *appended = 0;
    if (n == 0) {   // no valid pixel: a failed capture, skipped like main.py:53-54 (identity, empty statistics, nothing appended)
        for (int i = 0; i < 16; i++) T4x4[i] = (i % 5 == 0);
        if (stats) memset(stats, 0, sizeof *stats);
        return R3D_OK;
    }
    return model_align_core(m, ar, p, d_p, d_c, n, T4x4, stats, appended, t_begin, fbox);
}

int r3d_backproject_depth(r3d_ctx *ctx, const uint16_t *depth, int32_t w, int32_t h, int32_t stride, const r3d_depth_camera *cam,
                          const uint8_t *color, int32_t color_stride, double *out_xyz, double *out_colors, int32_t *out_pixel, int64_t *out_n) {
    R3D_ROCTX_RANGE("r3d_backproject_depth");
    if (!ctx) return R3D_E_BADARG;
    if (!out_xyz || !out_n || (color && !out_colors)) return r3d_fail(ctx, R3D_E_BADARG, "backproject_depth: bad argument");
    int rc;
    if ((rc = depth_args_ok(ctx, depth, w, h, stride, cam, color, color_stride, "backproject_depth"))) return rc;
    R3D_HIP(ctx, hipSetDevice(ctx->device));
    DevArena ar(ctx);
    double *d_p, *d_c;
    int *d_pix;
    int64_t n;
    if ((rc = backproject_core(ctx, ar, depth, w, h, stride, cam, color, color_stride, out_pixel != nullptr, &d_p, &d_c, &d_pix, &n))) return rc;
    *out_n = n;
    if (n == 0) return R3D_OK;
    if ((rc = r3d_download(ctx, out_xyz, d_p, (size_t)n * 3)) || (rc = r3d_download(ctx, out_colors, d_c, d_c ? (size_t)n * 3 : 0)) ||
        (rc = r3d_download(ctx, out_pixel, d_pix, (size_t)n)))
        return rc;
    R3D_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return R3D_OK;
}

int r3d_model_register_append(r3d_model *m, const r3d_icp_params *p, const double *src, const double *src_colors, const double *src_normals,
                              int64_t ns, double *T4x4, r3d_icp_stats *stats) {
    R3D_ROCTX_RANGE("r3d_model_register_append");
    if (!m) return R3D_E_BADARG;
    r3d_ctx *ctx = m->ctx;
    if (!p || !src || !T4x4 || ns <= 0) return r3d_fail(ctx, R3D_E_BADARG, "model_register_append: bad argument");
    if (m->n <= 0) return r3d_fail(ctx, R3D_E_BADARG, "model_register_append: the model is empty (append the first frame)");
    int rc;
    if ((rc = icp_mode_check(ctx, "model_register_append", p, m->has_normals, src_normals != nullptr, "the model has no normals (r3d_model_estimate_normals)")))
        return rc;
    R3D_HIP(ctx, hipSetDevice(ctx->device));
    const auto t_begin = std::chrono::steady_clock::now();
    DevArena ar(ctx);
    double *d_s, *d_c = nullptr, *d_sn = nullptr;
    if ((rc = upload(ctx, ar, src, ns * 3, &d_s)) || (rc = upload(ctx, ar, src_colors, ns * 3, &d_c)) || (rc = upload(ctx, ar, src_normals, ns * 3, &d_sn)))
        return rc;
    double T[16];
    const IcpInput in = {.d_s = d_s, .ns = ns, .d_sn = d_sn, .d_t = (const double *)m->pts.p, .nt = m->n,
                         .d_tn = m->has_normals ? (const double *)m->nrms.p : nullptr};
    if ((rc = icp_core(ctx, ar, p, in, T, stats, t_begin))) return rc;                 // test/GICP1.py:99-102, from identity
    memcpy(T4x4, T, sizeof T);
    double *d_o, *d_on;
    if ((rc = transform_cloud(ctx, ar, T, d_s, d_sn, ns, &d_o, &d_on))) return rc;    // :103 source.transform
    return model_append(m, d_o, d_c, d_on, ns, hipMemcpyDeviceToDevice);               // :146 combined += aligned
}

int r3d_model_estimate_normals(r3d_model *m, double radius, int32_t max_nn) {
    R3D_ROCTX_RANGE("r3d_model_estimate_normals");
    if (!m) return R3D_E_BADARG;
    r3d_ctx *ctx = m->ctx;
    if (max_nn < 1) return r3d_fail(ctx, R3D_E_BADARG, "model_estimate_normals: bad argument");
    if (max_nn > 128) return r3d_fail(ctx, R3D_E_UNSUPPORTED, "model_estimate_normals: max_nn > 128 not supported");
    if (m->n == 0) return R3D_OK;
    R3D_HIP(ctx, hipSetDevice(ctx->device));
    DevArena ar(ctx);
    int rc;
    double *d_n;
    // legacy EstimateNormals on a cloud that already has normals keeps their orientation (test/GICP1.py:148)
    if ((rc = normals_core(ctx, ar, (double *)m->pts.p, m->n, radius, max_nn, m->has_normals ? (double *)m->nrms.p : nullptr, &d_n))) return rc;
    if ((rc = model_rows(m, m->nrms, m->n, m->has_normals ? m->n : 0))) return rc;
    R3D_HIP(ctx, hipMemcpyAsync(m->nrms.p, d_n, (size_t)m->n * 24, hipMemcpyDeviceToDevice, ctx->stream));
    m->has_normals = true;
    return R3D_OK;
}

int r3d_model_download(r3d_model *m, double *xyz, double *colors, double *normals) {
    R3D_ROCTX_RANGE("r3d_model_download");
    if (!m) return R3D_E_BADARG;
    r3d_ctx *ctx = m->ctx;
    if (!xyz) return r3d_fail(ctx, R3D_E_BADARG, "model_download: bad argument");
    if (m->n == 0) return R3D_OK;
    R3D_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n3 = (size_t)m->n * 3;
    if (int rc = r3d_download(ctx, xyz, (const double *)m->pts.p, n3)) return rc;
    if (int rc = r3d_download(ctx, colors, (const double *)m->cols.p, m->has_colors ? n3 : 0)) return rc;
    if (int rc = r3d_download(ctx, normals, (const double *)m->nrms.p, m->has_normals ? n3 : 0)) return rc;
    R3D_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return R3D_OK;
}

// Device-pointer forms for callers that keep their clouds in HBM (the multi-view exchange of config C5: clouds produced by
// r3d_disparity_to_cloud_resident, gathered by RCCL, registered and transformed without touching the host).  Work is enqueued on
// the context stream; r3d_icp_dev returns when the loop has finished (it reads the state back), r3d_transform_points_dev is
// asynchronous.
int r3d_icp_dev(r3d_ctx *ctx, const r3d_icp_params *p, const double *d_src, int64_t ns, const double *d_src_normals, const double *d_tgt,
                int64_t nt, const double *d_tgt_normals, const double *init4x4, double *T4x4, r3d_icp_stats *stats) {
    R3D_ROCTX_RANGE("r3d_icp_dev");
    if (!ctx) return R3D_E_BADARG;
    if (!p || !d_src || !d_tgt || !T4x4 || ns <= 0 || nt <= 0) return r3d_fail(ctx, R3D_E_BADARG, "icp_dev: bad argument");
    if (int rc = icp_mode_check(ctx, "icp_dev", p, d_tgt_normals != nullptr, d_src_normals != nullptr)) return rc;
    R3D_HIP(ctx, hipSetDevice(ctx->device));
    const auto t_begin = std::chrono::steady_clock::now();
    DevArena ar(ctx);
    const IcpInput in = {.d_s = d_src, .ns = ns, .d_sn = d_src_normals, .d_t = d_tgt, .nt = nt, .d_tn = d_tgt_normals, .init4x4 = init4x4};
    return icp_core(ctx, ar, p, in, T4x4, stats, t_begin);
}

// ---- coloured ICP (Open3D registration_colored_icp): the intensity gradients on their own, and the registration on host / device clouds
int r3d_color_gradients(r3d_ctx *ctx, const double *xyz, const double *normals, const double *colors, int64_t n, double radius, int32_t max_nn,
                        double *out_intensity, double *out_gradient) {
    R3D_ROCTX_RANGE("r3d_color_gradients");
    if (!ctx) return R3D_E_BADARG;
    if (!xyz || !normals || !colors || !out_intensity || !out_gradient || n <= 0) return r3d_fail(ctx, R3D_E_BADARG, "color_gradients: bad argument");
    if (!(radius > 0)) return r3d_fail(ctx, R3D_E_BADARG, "color_gradients: radius must be > 0 (the search is a hybrid one)");
    if (max_nn < 1 || max_nn > 128) return r3d_fail(ctx, R3D_E_BADARG, "color_gradients: max_nn must be in 1..128");
    R3D_HIP(ctx, hipSetDevice(ctx->device));
    DevArena ar(ctx);
    double *d_p, *d_n, *d_c, *d_rec;
    int rc;
    if ((rc = upload(ctx, ar, xyz, n * 3, &d_p)) || (rc = upload(ctx, ar, normals, n * 3, &d_n)) || (rc = upload(ctx, ar, colors, n * 3, &d_c))) return rc;
    if ((rc = color_gradients_core(ctx, ar, d_p, n, d_n, d_c, radius, max_nn, &d_rec))) return rc;
    std::vector<double> rec((size_t)n * 4);
    R3D_HIP(ctx, hipMemcpyAsync(rec.data(), d_rec, (size_t)n * 32, hipMemcpyDeviceToHost, ctx->stream));
    R3D_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (int64_t i = 0; i < n; i++) {
        out_intensity[i] = rec[i * 4];
        out_gradient[i * 3] = rec[i * 4 + 1]; out_gradient[i * 3 + 1] = rec[i * 4 + 2]; out_gradient[i * 3 + 2] = rec[i * 4 + 3];
    }
    return R3D_OK;
}

// argument checks shared by the two coloured entry points; fills the resolved parameters
static int colored_icp_check(r3d_ctx *ctx, const char *who, const r3d_colored_icp_params *p, const void *src, const void *src_colors, int64_t ns,
                             const void *tgt, const void *tgt_normals, const void *tgt_colors, int64_t nt, const double *T4x4, r3d_icp_params *ip,
                             IcpColorInput *ci) {
    if (!p || !src || !tgt || !T4x4 || ns <= 0 || nt <= 0) return r3d_fail(ctx, R3D_E_BADARG, "%s: bad argument", who);
    if (p->icp.mode != MODE_COLORED) return r3d_fail(ctx, R3D_E_BADARG, "%s: icp.mode must be R3D_ICP_COLORED (3)", who);
    if (!(p->icp.max_correspondence_distance > 0)) return r3d_fail(ctx, R3D_E_BADARG, "%s: max_correspondence_distance must be > 0", who);
    if (!src_colors || !tgt_colors) return r3d_fail(ctx, R3D_E_BADARG, "%s: source and target colours required", who);
    if (!tgt_normals) return r3d_fail(ctx, R3D_E_BADARG, "%s: target normals required", who);
    if (!(p->lambda_geometric >= 0.0 && p->lambda_geometric <= 1.0)) return r3d_fail(ctx, R3D_E_BADARG, "%s: lambda_geometric must lie in [0, 1]", who);
    if (p->gradient_max_nn > 128) return r3d_fail(ctx, R3D_E_BADARG, "%s: gradient_max_nn > 128 not supported", who);
    *ip = p->icp;
    ci->d_sc = ci->d_tc = nullptr;
    ci->lambda = p->lambda_geometric;
    ci->radius = p->gradient_radius > 0 ? p->gradient_radius : 2.0 * p->icp.max_correspondence_distance;
    ci->max_nn = p->gradient_max_nn > 0 ? p->gradient_max_nn : 30;
    return R3D_OK;
}

int r3d_icp_colored(r3d_ctx *ctx, const r3d_colored_icp_params *p, const double *src, const double *src_colors, int64_t ns, const double *tgt,
                    const double *tgt_normals, const double *tgt_colors, int64_t nt, const double *init4x4, double *T4x4, r3d_icp_stats *stats) {
    R3D_ROCTX_RANGE("r3d_icp_colored");
    if (!ctx) return R3D_E_BADARG;
    r3d_icp_params ip;
    IcpColorInput ci;
    int rc;
    if ((rc = colored_icp_check(ctx, "icp_colored", p, src, src_colors, ns, tgt, tgt_normals, tgt_colors, nt, T4x4, &ip, &ci))) return rc;
    R3D_HIP(ctx, hipSetDevice(ctx->device));
    const auto t_begin = std::chrono::steady_clock::now();
    DevArena ar(ctx);
    double *d_t, *d_tn, *d_tc, *d_s, *d_sc;
    if ((rc = upload_pair(ctx, ar, src, ns, tgt, nt, &d_s, &d_t)) || (rc = upload(ctx, ar, tgt_normals, nt * 3, &d_tn)) ||
        (rc = upload(ctx, ar, tgt_colors, nt * 3, &d_tc)) || (rc = upload(ctx, ar, src_colors, ns * 3, &d_sc)))
        return rc;
    ci.d_sc = d_sc; ci.d_tc = d_tc;
    return icp_core(ctx, ar, &ip, {.d_s = d_s, .ns = ns, .d_t = d_t, .nt = nt, .d_tn = d_tn, .init4x4 = init4x4, .color = &ci}, T4x4, stats, t_begin);
}

int r3d_icp_colored_dev(r3d_ctx *ctx, const r3d_colored_icp_params *p, const double *d_src, const double *d_src_colors, int64_t ns, const double *d_tgt,
                        const double *d_tgt_normals, const double *d_tgt_colors, int64_t nt, const double *init4x4, double *T4x4, r3d_icp_stats *stats) {
    R3D_ROCTX_RANGE("r3d_icp_colored_dev");
    if (!ctx) return R3D_E_BADARG;
    r3d_icp_params ip;
    IcpColorInput ci;
    int rc;
    if ((rc = colored_icp_check(ctx, "icp_colored_dev", p, d_src, d_src_colors, ns, d_tgt, d_tgt_normals, d_tgt_colors, nt, T4x4, &ip, &ci))) return rc;
    R3D_HIP(ctx, hipSetDevice(ctx->device));
    const auto t_begin = std::chrono::steady_clock::now();
    DevArena ar(ctx);
    ci.d_sc = d_src_colors; ci.d_tc = d_tgt_colors;
    const IcpInput in = {.d_s = d_src, .ns = ns, .d_t = d_tgt, .nt = nt, .d_tn = d_tgt_normals, .init4x4 = init4x4, .color = &ci};
    return icp_core(ctx, ar, &ip, in, T4x4, stats, t_begin);
}

// ---- FPFH features and feature-space nearest neighbours (Open3D compute_fpfh_feature / CorrespondencesFromFeatures' search)
static int fpfh_check(r3d_ctx *ctx, const char *who, const void *xyz, const void *in2, const void *out, int64_t n, int32_t max_nn) {
    if (!xyz || !in2 || !out || n <= 0 || max_nn < 1) return r3d_fail(ctx, R3D_E_BADARG, "%s: bad argument (null array, n <= 0 or max_nn < 1)", who);
    if (max_nn > 128) return r3d_fail(ctx, R3D_E_UNSUPPORTED, "%s: max_nn > 128 not supported", who);
    return R3D_OK;
}

int r3d_compute_fpfh_dev(r3d_ctx *ctx, const double *d_xyz, const double *d_normals, int64_t n, double radius, int32_t max_nn, double *d_fpfh,
                         double *d_spfh) {
    R3D_ROCTX_RANGE("r3d_compute_fpfh_dev");
    if (!ctx) return R3D_E_BADARG;
    if (int rc = fpfh_check(ctx, "compute_fpfh_dev", d_xyz, d_normals, d_fpfh, n, max_nn)) return rc;
    R3D_HIP(ctx, hipSetDevice(ctx->device));
    DevArena ar(ctx);
    return fpfh_core(ctx, ar, d_xyz, d_normals, nullptr, n, radius, max_nn, d_fpfh, d_spfh);
}

int r3d_compute_fpfh(r3d_ctx *ctx, const double *xyz, const double *normals, int64_t n, double radius, int32_t max_nn, double *fpfh, double *spfh) {
    R3D_ROCTX_RANGE("r3d_compute_fpfh");
    if (!ctx) return R3D_E_BADARG;
    int rc;
    if ((rc = fpfh_check(ctx, "compute_fpfh", xyz, normals, fpfh, n, max_nn))) return rc;
    R3D_HIP(ctx, hipSetDevice(ctx->device));
    DevArena ar(ctx);
    double *d_p, *d_n;
    if ((rc = upload(ctx, ar, xyz, n * 3, &d_p)) || (rc = upload(ctx, ar, normals, n * 3, &d_n))) return rc;
    double *d_f = (double *)ar.get((size_t)n * FPFH_DIM * 8), *d_s = spfh ? (double *)ar.get((size_t)n * FPFH_DIM * 8) : nullptr;
    if (ar.rc) return ar.rc;
    if ((rc = fpfh_core(ctx, ar, d_p, d_n, nullptr, n, radius, max_nn, d_f, d_s))) return rc;
    if ((rc = r3d_download(ctx, fpfh, d_f, (size_t)n * FPFH_DIM)) || (rc = r3d_download(ctx, spfh, d_s, (size_t)n * FPFH_DIM))) return rc;
    R3D_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return R3D_OK;
}

int r3d_fpfh_from_spfh(r3d_ctx *ctx, const double *xyz, int64_t n, double radius, int32_t max_nn, const double *spfh_in, double *fpfh) {
    R3D_ROCTX_RANGE("r3d_fpfh_from_spfh");
    if (!ctx) return R3D_E_BADARG;
    int rc;
    if ((rc = fpfh_check(ctx, "fpfh_from_spfh", xyz, spfh_in, fpfh, n, max_nn))) return rc;
    R3D_HIP(ctx, hipSetDevice(ctx->device));
    DevArena ar(ctx);
    double *d_p, *d_s;
    if ((rc = upload(ctx, ar, xyz, n * 3, &d_p)) || (rc = upload(ctx, ar, spfh_in, n * FPFH_DIM, &d_s))) return rc;
    double *d_f = (double *)ar.get((size_t)n * FPFH_DIM * 8);
    if (ar.rc) return ar.rc;
    if ((rc = fpfh_core(ctx, ar, d_p, nullptr, d_s, n, radius, max_nn, d_f, nullptr))) return rc;
    if ((rc = r3d_download(ctx, fpfh, d_f, (size_t)n * FPFH_DIM))) return rc;
    R3D_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return R3D_OK;
}

static int match_check(r3d_ctx *ctx, const char *who, const void *src, int64_t ns, const void *tgt, int64_t nt, int32_t dim, const void *nn_out) {
    if (!src || !tgt || !nn_out || ns <= 0 || nt <= 0) return r3d_fail(ctx, R3D_E_BADARG, "%s: bad argument", who);
    if (dim != FPFH_DIM) return r3d_fail(ctx, R3D_E_UNSUPPORTED, "%s: dim = %d not supported (FPFH rows have 33 entries)", who, dim);
    if (ns > 0x7fffffff || nt > 0x7fffffff || (double)ns * (double)nt > MATCH_MAX_PAIRS)
        return r3d_fail(ctx, R3D_E_UNSUPPORTED, "%s: %lld x %lld rows is more than the brute-force search takes on (ns * nt <= %.0e)", who,
                        (long long)ns, (long long)nt, MATCH_MAX_PAIRS);
    return R3D_OK;
}

int r3d_match_features_dev(r3d_ctx *ctx, const double *d_src_feat, int64_t ns, const double *d_tgt_feat, int64_t nt, int32_t dim, int32_t *d_nn_out,
                           double *d_d2_out) {
    R3D_ROCTX_RANGE("r3d_match_features_dev");
    if (!ctx) return R3D_E_BADARG;
    if (int rc = match_check(ctx, "match_features_dev", d_src_feat, ns, d_tgt_feat, nt, dim, d_nn_out)) return rc;
    R3D_HIP(ctx, hipSetDevice(ctx->device));
    DevArena ar(ctx);
    return match_core(ctx, ar, d_src_feat, ns, d_tgt_feat, nt, d_nn_out, d_d2_out);
}

int r3d_match_features(r3d_ctx *ctx, const double *src_feat, int64_t ns, const double *tgt_feat, int64_t nt, int32_t dim, int32_t *nn_out,
                       double *d2_out) {
    R3D_ROCTX_RANGE("r3d_match_features");
    if (!ctx) return R3D_E_BADARG;
    int rc;
    if ((rc = match_check(ctx, "match_features", src_feat, ns, tgt_feat, nt, dim, nn_out))) return rc;
    R3D_HIP(ctx, hipSetDevice(ctx->device));
    DevArena ar(ctx);
    double *d_s, *d_t;
    if ((rc = upload_pair(ctx, ar, src_feat, ns, tgt_feat, nt, &d_s, &d_t, FPFH_DIM))) return rc;
    int *d_nn = (int *)ar.get((size_t)ns * 4);
    double *d_d2 = d2_out ? (double *)ar.get((size_t)ns * 8) : nullptr;
    if (ar.rc) return ar.rc;
    if ((rc = match_core(ctx, ar, d_s, ns, d_t, nt, d_nn, d_d2))) return rc;
    if ((rc = r3d_download(ctx, nn_out, d_nn, (size_t)ns)) || (rc = r3d_download(ctx, d2_out, d_d2, (size_t)ns))) return rc;
    R3D_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return R3D_OK;
}

// diagnostic (tools/gpu_bench_fpfh.py): the stages of r3d_compute_fpfh_dev timed with events in one call, next to k_knn_graph at
// the same (n, k, radius) on the same grid -- the search both feature stages share.  ms[0] k_knn_graph, ms[1] k_spfh (with the
// gather of the normals), ms[2] k_fpfh.  Synchronises.
int r3d_debug_fpfh_stages(r3d_ctx *ctx, const double *d_xyz, const double *d_normals, int64_t n, double radius, int32_t max_nn, double *d_fpfh,
                          float *ms3) {
    if (!ctx) return R3D_E_BADARG;
    int rc;
    if (!ms3) return r3d_fail(ctx, R3D_E_BADARG, "debug_fpfh_stages: bad argument");
    if ((rc = fpfh_check(ctx, "debug_fpfh_stages", d_xyz, d_normals, d_fpfh, n, max_nn))) return rc;
    R3D_HIP(ctx, hipSetDevice(ctx->device));
    r3d_events<5> ev;
    R3D_HIP(ctx, ev.create_all());
    {
        DevArena ar(ctx);
        rc = fpfh_core(ctx, ar, d_xyz, d_normals, nullptr, n, radius, max_nn, d_fpfh, nullptr, ev.e);
    }
    if (!rc) {
        DevArena ar(ctx);
        Grid G;
        const int k = (int)std::min<int64_t>(max_nn, n);
        if (!(rc = grid_build(ctx, ar, d_xyz, n, radius, knn_target_occ(k), G))) {
            int *d_nb = (int *)ar.get((size_t)n * k * 4);
            double *d_d2 = (double *)ar.get((size_t)n * k * 8);
            if (!(rc = ar.rc)) {
                (void)hipEventRecord(ev[3], ctx->stream);
                rc = launch_knn(ctx, k_knn_graph, G, n, k, radius, d_nb, d_d2);
                (void)hipEventRecord(ev[4], ctx->stream);
            }
        }
    }
    hipError_t e = hipStreamSynchronize(ctx->stream);
    if (!rc && e == hipSuccess) {
        (void)hipEventElapsedTime(&ms3[0], ev[3], ev[4]);
        (void)hipEventElapsedTime(&ms3[1], ev[0], ev[1]);
        (void)hipEventElapsedTime(&ms3[2], ev[1], ev[2]);
    }
    if (rc) return rc;
    if (e != hipSuccess) return r3d_fail(ctx, R3D_E_HIP, "debug_fpfh_stages: %s", hipGetErrorString(e));
    return R3D_OK;
}

// ---- feature-matching RANSAC over given correspondences (Open3D registration_ransac_based_on_correspondence)
int r3d_ransac_correspondence_dev(r3d_ctx *ctx, const r3d_ransac_params *p, const double *d_src, int64_t ns, const double *d_tgt, int64_t nt,
                                  const int32_t *d_corres, int64_t M, double *T4x4, uint8_t *d_inlier_mask, r3d_ransac_stats *stats) {
    R3D_ROCTX_RANGE("r3d_ransac_correspondence_dev");
    if (!ctx) return R3D_E_BADARG;
    const auto t_begin = std::chrono::steady_clock::now();
    if (!T4x4) return r3d_fail(ctx, R3D_E_BADARG, "ransac_correspondence_dev: T4x4 is NULL");
    if (int rc = ransac_check(ctx, "ransac_correspondence_dev", p, d_src, ns, d_tgt, nt, d_corres, M)) return rc;
    R3D_HIP(ctx, hipSetDevice(ctx->device));
    DevArena ar(ctx);
    return ransac_core(ctx, ar, p, d_src, ns, d_tgt, nt, d_corres, M, T4x4, d_inlier_mask, nullptr, stats, t_begin);
}

int r3d_ransac_correspondence(r3d_ctx *ctx, const r3d_ransac_params *p, const double *src, int64_t ns, const double *tgt, int64_t nt,
                              const int32_t *corres, int64_t M, double *T4x4, uint8_t *inlier_mask, r3d_ransac_stats *stats) {
    R3D_ROCTX_RANGE("r3d_ransac_correspondence");
    if (!ctx) return R3D_E_BADARG;
    const auto t_begin = std::chrono::steady_clock::now();
    int rc;
    if (!T4x4) return r3d_fail(ctx, R3D_E_BADARG, "ransac_correspondence: T4x4 is NULL");
    if ((rc = ransac_check(ctx, "ransac_correspondence", p, src, ns, tgt, nt, corres, M))) return rc;
    R3D_HIP(ctx, hipSetDevice(ctx->device));
    DevArena ar(ctx);
    double *d_s, *d_t;
    int *d_c;
    if ((rc = upload_corres_problem(ctx, ar, src, ns, tgt, nt, corres, M, &d_s, &d_t, &d_c))) return rc;
    return ransac_core(ctx, ar, p, d_s, ns, d_t, nt, d_c, M, T4x4, nullptr, inlier_mask, stats, t_begin);
}

int r3d_debug_ransac_hypotheses(r3d_ctx *ctx, const r3d_ransac_params *p, const double *src, int64_t ns, const double *tgt, int64_t nt,
                                const int32_t *corres, int64_t M, int64_t h0, int64_t count, int32_t *samples, int32_t *flags, double *T,
                                int32_t *inliers, double *err2) {
    R3D_ROCTX_RANGE("r3d_debug_ransac_hypotheses");
    if (!ctx) return R3D_E_BADARG;
    int rc;
    if ((rc = ransac_check(ctx, "debug_ransac_hypotheses", p, src, ns, tgt, nt, corres, M))) return rc;
    if (h0 < 0 || count < 1 || count > RANSAC_MAX_BATCH || h0 + count > 0x7fffffff)
        return r3d_fail(ctx, R3D_E_BADARG, "debug_ransac_hypotheses: h0 >= 0, 1 <= count <= %d, h0 + count < 2^31", RANSAC_MAX_BATCH);
    R3D_HIP(ctx, hipSetDevice(ctx->device));
    DevArena ar(ctx);
    double *d_s, *d_t;
    int *d_c;
    if ((rc = upload_corres_problem(ctx, ar, src, ns, tgt, nt, corres, M, &d_s, &d_t, &d_c))) return rc;
    RansacWork W;
    const int n = (int)count;
    if ((rc = ransac_setup(ctx, ar, d_s, ns, d_t, nt, d_c, M, n, true, W))) return rc;
    RansacDev pd = ransac_dev_params(p);
    pd.h0 = h0;
    pd.count = n;
    int nsurv = 0;
    if ((rc = ransac_batch(ctx, ar, W, M, pd, &nsurv))) return rc;
    std::vector<int> surv, cnt, fl(n);
    std::vector<double> err, Ts((size_t)n * 12);
    if (nsurv > 0 && (rc = ransac_read_results(ctx, W, nsurv, surv, cnt, err))) return rc;
    if ((rc = r3d_download(ctx, samples, W.samples, (size_t)n * 4)) || (rc = r3d_download(ctx, fl.data(), W.flags, (size_t)n)) ||
        (rc = r3d_download(ctx, Ts.data(), W.T, (size_t)n * 12)))
        return rc;
    R3D_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (int i = 0; i < n; i++) {
        if (flags) flags[i] = fl[i];
        if (T) for (int e = 0; e < 12; e++) T[(size_t)i * 12 + e] = (fl[i] & 1) ? Ts[(size_t)e * n + i] : 0.0;   // slots of rejected samples hold an earlier call's values
        if (inliers) inliers[i] = 0;
        if (err2) err2[i] = 0.0;
    }
    for (int k = 0; k < nsurv; k++) {
        if (inliers) inliers[surv[k]] = cnt[k];
        if (err2) err2[surv[k]] = err[k];
    }
    return R3D_OK;
}

// ---- Fast Global Registration (Open3D registration_fgr_based_on_correspondence / ..._on_feature_matching)
static int fgr_pairs_check(r3d_ctx *ctx, const char *who, const void *corres, int64_t M) {
    if (!corres || M < 0) return r3d_fail(ctx, R3D_E_BADARG, "%s: bad argument (no correspondences)", who);
    if (M > 0x7fffffff) return r3d_fail(ctx, R3D_E_UNSUPPORTED, "%s: M must stay below 2^31", who);
    return R3D_OK;
}

int r3d_fgr_correspondence_dev(r3d_ctx *ctx, const r3d_fgr_params *p, const double *d_src, int64_t ns, const double *d_tgt, int64_t nt,
                               const int32_t *d_corres, int64_t M, double *T4x4, r3d_fgr_stats *stats) {
    R3D_ROCTX_RANGE("r3d_fgr_correspondence_dev");
    if (!ctx) return R3D_E_BADARG;
    const auto t_begin = std::chrono::steady_clock::now();
    int rc;
    if (!T4x4) return r3d_fail(ctx, R3D_E_BADARG, "fgr_correspondence_dev: T4x4 is NULL");
    if ((rc = fgr_check(ctx, "fgr_correspondence_dev", p, d_src, ns, d_tgt, nt)) || (rc = fgr_pairs_check(ctx, "fgr_correspondence_dev", d_corres, M)))
        return rc;
    R3D_HIP(ctx, hipSetDevice(ctx->device));
    DevArena ar(ctx);
    return fgr_core(ctx, ar, p, d_src, ns, d_tgt, nt, d_corres, M, nullptr, nullptr, T4x4, stats, t_begin);
}

int r3d_fgr_correspondence(r3d_ctx *ctx, const r3d_fgr_params *p, const double *src, int64_t ns, const double *tgt, int64_t nt,
                           const int32_t *corres, int64_t M, double *T4x4, r3d_fgr_stats *stats) {
    R3D_ROCTX_RANGE("r3d_fgr_correspondence");
    if (!ctx) return R3D_E_BADARG;
    const auto t_begin = std::chrono::steady_clock::now();
    int rc;
    if (!T4x4) return r3d_fail(ctx, R3D_E_BADARG, "fgr_correspondence: T4x4 is NULL");
    if ((rc = fgr_check(ctx, "fgr_correspondence", p, src, ns, tgt, nt)) || (rc = fgr_pairs_check(ctx, "fgr_correspondence", corres, M))) return rc;
    R3D_HIP(ctx, hipSetDevice(ctx->device));
    DevArena ar(ctx);
    double *d_s, *d_t;
    int *d_c;
    if ((rc = upload_corres_problem(ctx, ar, src, ns, tgt, nt, corres, M, &d_s, &d_t, &d_c))) return rc;
    return fgr_core(ctx, ar, p, d_s, ns, d_t, nt, d_c, M, nullptr, nullptr, T4x4, stats, t_begin);
}

int r3d_fgr_feature_matching_dev(r3d_ctx *ctx, const r3d_fgr_params *p, const double *d_src, int64_t ns, const double *d_tgt, int64_t nt,
                                 const double *d_src_feat, const double *d_tgt_feat, int32_t dim, double *T4x4, r3d_fgr_stats *stats) {
    R3D_ROCTX_RANGE("r3d_fgr_feature_matching_dev");
    if (!ctx) return R3D_E_BADARG;
    const auto t_begin = std::chrono::steady_clock::now();
    int rc;
    if (!T4x4) return r3d_fail(ctx, R3D_E_BADARG, "fgr_feature_matching_dev: T4x4 is NULL");
    if ((rc = fgr_check(ctx, "fgr_feature_matching_dev", p, d_src, ns, d_tgt, nt))) return rc;
    if ((rc = match_check(ctx, "fgr_feature_matching_dev", d_src_feat, ns, d_tgt_feat, nt, dim, T4x4))) return rc;
    R3D_HIP(ctx, hipSetDevice(ctx->device));
    DevArena ar(ctx);
    return fgr_core(ctx, ar, p, d_src, ns, d_tgt, nt, nullptr, 0, d_src_feat, d_tgt_feat, T4x4, stats, t_begin);
}

int r3d_fgr_feature_matching(r3d_ctx *ctx, const r3d_fgr_params *p, const double *src, int64_t ns, const double *tgt, int64_t nt,
                             const double *src_feat, const double *tgt_feat, int32_t dim, double *T4x4, r3d_fgr_stats *stats) {
    R3D_ROCTX_RANGE("r3d_fgr_feature_matching");
    if (!ctx) return R3D_E_BADARG;
    const auto t_begin = std::chrono::steady_clock::now();
    int rc;
    if (!T4x4) return r3d_fail(ctx, R3D_E_BADARG, "fgr_feature_matching: T4x4 is NULL");
    if ((rc = fgr_check(ctx, "fgr_feature_matching", p, src, ns, tgt, nt))) return rc;
    if ((rc = match_check(ctx, "fgr_feature_matching", src_feat, ns, tgt_feat, nt, dim, T4x4))) return rc;
    R3D_HIP(ctx, hipSetDevice(ctx->device));
    DevArena ar(ctx);
    double *d_s, *d_t, *d_sf, *d_tf;
    if ((rc = upload_pair(ctx, ar, src, ns, tgt, nt, &d_s, &d_t)) || (rc = upload_pair(ctx, ar, src_feat, ns, tgt_feat, nt, &d_sf, &d_tf, FPFH_DIM))) return rc;
    return fgr_core(ctx, ar, p, d_s, ns, d_t, nt, nullptr, 0, d_sf, d_tf, T4x4, stats, t_begin);
}

// stage parity: trials t0 .. t0 + count - 1 of the tuple test over the normalised pairs, without the cut
int r3d_debug_fgr_tuples(r3d_ctx *ctx, const r3d_fgr_params *p, const double *src, int64_t ns, const double *tgt, int64_t nt, const int32_t *corres,
                         int64_t M, int64_t t0, int64_t count, int32_t *samples, int32_t *flags) {
    R3D_ROCTX_RANGE("r3d_debug_fgr_tuples");
    if (!ctx) return R3D_E_BADARG;
    int rc;
    if ((rc = fgr_check(ctx, "debug_fgr_tuples", p, src, ns, tgt, nt)) || (rc = fgr_pairs_check(ctx, "debug_fgr_tuples", corres, M))) return rc;
    if (M < 1 || t0 < 0 || count < 1 || count > RANSAC_MAX_BATCH || t0 > (int64_t)1 << 60)
        return r3d_fail(ctx, R3D_E_BADARG, "debug_fgr_tuples: M >= 1, t0 >= 0, 1 <= count <= %d", RANSAC_MAX_BATCH);
    R3D_HIP(ctx, hipSetDevice(ctx->device));
    DevArena ar(ctx);
    double *d_s, *d_t;
    int *d_c;
    if ((rc = upload_corres_problem(ctx, ar, src, ns, tgt, nt, corres, M, &d_s, &d_t, &d_c))) return rc;
    FgrNorm nm;
    double scale_start, *rows;
    if ((rc = fgr_normalise(ctx, ar, d_s, ns, d_t, nt, p->use_absolute_scale != 0, nm, &scale_start))) return rc;
    if ((rc = fgr_gather(ctx, ar, d_s, ns, d_t, nt, d_c, M, nm, &rows))) return rc;
    const int n = (int)count;
    int *d_samples = (int *)ar.get((size_t)n * 12), *d_flags = (int *)ar.get((size_t)(n + 1) * 4);
    if (ar.rc) return ar.rc;
    k_fgr_tuples<<<(unsigned)((n + 255) / 256), 256, 0, ctx->stream>>>(rows, M, p->seed, t0, n, p->tuple_scale, d_samples, d_flags, nullptr);
    R3D_HIP(ctx, hipGetLastError());
    if ((rc = r3d_download(ctx, samples, d_samples, (size_t)n * 3)) || (rc = r3d_download(ctx, flags, d_flags, (size_t)n))) return rc;
    R3D_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return R3D_OK;
}

// stage parity: step 4 alone on the given pairs (no tuple test), the state after every iteration in normalised units
int r3d_debug_fgr_optimize(r3d_ctx *ctx, const r3d_fgr_params *p, const double *src, int64_t ns, const double *tgt, int64_t nt, const int32_t *pairs,
                           int64_t M, double *trace_T, double *trace_par) {
    R3D_ROCTX_RANGE("r3d_debug_fgr_optimize");
    if (!ctx) return R3D_E_BADARG;
    int rc;
    if ((rc = fgr_check(ctx, "debug_fgr_optimize", p, src, ns, tgt, nt)) || (rc = fgr_pairs_check(ctx, "debug_fgr_optimize", pairs, M))) return rc;
    if (p->iteration_number > 0 && (!trace_T || !trace_par)) return r3d_fail(ctx, R3D_E_BADARG, "debug_fgr_optimize: trace_T or trace_par is NULL");
    R3D_HIP(ctx, hipSetDevice(ctx->device));
    DevArena ar(ctx);
    double *d_s, *d_t;
    int *d_c;
    if ((rc = upload_corres_problem(ctx, ar, src, ns, tgt, nt, pairs, M, &d_s, &d_t, &d_c))) return rc;
    FgrNorm nm;
    double scale_start, *rows, trans[16], final_par;
    if ((rc = fgr_normalise(ctx, ar, d_s, ns, d_t, nt, p->use_absolute_scale != 0, nm, &scale_start))) return rc;
    if ((rc = fgr_gather(ctx, ar, d_s, ns, d_t, nt, d_c, M, nm, &rows))) return rc;
    return fgr_optimise_stage(ctx, ar, p, rows, M, scale_start, trans, &final_par, trace_T, trace_par);
}

int r3d_transform_points_dev(r3d_ctx *ctx, const double *d_xyz, int64_t n, const double *T4x4, int32_t rotate_only, double *d_out) {
    R3D_ROCTX_RANGE("r3d_transform_points_dev");
    if (!ctx) return R3D_E_BADARG;
    if (!d_xyz || !d_out || !T4x4 || n < 0) return r3d_fail(ctx, R3D_E_BADARG, "transform_points_dev: bad argument");
    if (n == 0) return R3D_OK;
    R3D_HIP(ctx, hipSetDevice(ctx->device));
    k_transform<<<(unsigned)((n + 255) / 256), 256, 0, ctx->stream>>>(d_xyz, n, to_rigid(T4x4), rotate_only, d_out);
    R3D_HIP(ctx, hipGetLastError());
    return R3D_OK;
}

int r3d_transform_blocks_dev(r3d_ctx *ctx, int32_t n_blocks, const double *const *d_xyz, const int64_t *counts, const double *T4x4s,
                             const int32_t *rotate_only, double *const *d_out) {
    R3D_ROCTX_RANGE("r3d_transform_blocks_dev");
    if (!ctx) return R3D_E_BADARG;
    if (n_blocks < 0 || (n_blocks > 0 && (!d_xyz || !counts || !T4x4s || !d_out))) return r3d_fail(ctx, R3D_E_BADARG, "transform_blocks_dev: bad argument");
    for (int b = 0; b < n_blocks; b++)
        if (counts[b] < 0 || (counts[b] > 0 && (!d_xyz[b] || !d_out[b]))) return r3d_fail(ctx, R3D_E_BADARG, "transform_blocks_dev: block %d: bad argument", b);
    R3D_HIP(ctx, hipSetDevice(ctx->device));
    for (int b = 0; b < n_blocks;) {
        TransformBlocks B;
        B.n = 0;
        long long end = 0;
        for (; b < n_blocks && B.n < TB_MAX; b++) {   // the next TB_MAX non-empty blocks
            if (counts[b] == 0) continue;
            const double *T = T4x4s + (size_t)b * 16;
            const bool ro = rotate_only && rotate_only[b];
            const int q = B.n++;
            B.in[q] = d_xyz[b];
            B.out[q] = d_out[b];
            end += counts[b];
            B.end[q] = end;
            for (int i = 0; i < 3; i++) {
                for (int j = 0; j < 3; j++) B.r[q][i * 3 + j] = T[i * 4 + j];
                B.r[q][9 + i] = ro ? 0.0 : T[i * 4 + 3];
            }
        }
        if (B.n == 0) continue;
        for (int q = B.n; q < TB_MAX; q++) { B.in[q] = nullptr; B.out[q] = nullptr; B.end[q] = end; }
        k_transform_blocks<<<(unsigned)((end + 255) / 256), 256, 0, ctx->stream>>>(B);
        R3D_HIP(ctx, hipGetLastError());
    }
    return R3D_OK;
}

}  // extern "C"

// diagnostic: the cell sort on its own (tests compare both implementations with a host lexsort)
extern "C" int r3d_debug_sort_by_cell(r3d_ctx *ctx, const double *xyz, int64_t n, const double *org3, double cell, const int32_t *dims3, int32_t key_order,
                                      int32_t impl, int32_t *idx_out, uint64_t *keys_out) {
    R3D_ROCTX_RANGE("r3d_debug_sort_by_cell");
    if (!ctx) return R3D_E_BADARG;
    if (!xyz || !org3 || !dims3 || !idx_out || n <= 0 || !(cell > 0) || key_order < 0 || key_order > 3 || impl < 0 || impl > 1)
        return r3d_fail(ctx, R3D_E_BADARG, "debug_sort_by_cell: bad argument");
    R3D_HIP(ctx, hipSetDevice(ctx->device));
    DevArena ar(ctx);
    double *d_p;
    int rc;
    if ((rc = upload(ctx, ar, xyz, n * 3, &d_p))) return rc;
    const int dims[3] = {dims3[0], dims3[1], dims3[2]};
    void *keys;
    bool k32;
    int *idx;
    if ((rc = sort_by_cell(ctx, ar, d_p, n, org3, cell, dims, key_order, &keys, &k32, &idx, nullptr, impl))) return rc;
    if ((rc = r3d_download(ctx, idx_out, idx, (size_t)n))) return rc;
    std::vector<unsigned> k4;
    if (keys_out) {
        if (k32) {
            k4.resize((size_t)n);
            R3D_HIP(ctx, hipMemcpyAsync(k4.data(), keys, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
        } else if ((rc = r3d_download(ctx, keys_out, (const uint64_t *)keys, (size_t)n))) return rc;
    }
    R3D_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (keys_out && k32)
        for (int64_t i = 0; i < n; i++) keys_out[i] = k4[(size_t)i];
    return R3D_OK;
}

// diagnostic: the registration's correspondence search on its own -- icp_core's set-up (point-to-point), one evaluation at pose T
extern "C" int r3d_debug_icp_correspondences(r3d_ctx *ctx, const double *src, int64_t ns, const double *tgt, int64_t nt,
                                             double max_correspondence_distance, const double *T4x4, int32_t *corr_out, double *d2_out) {
    R3D_ROCTX_RANGE("r3d_debug_icp_correspondences");
    if (!ctx) return R3D_E_BADARG;
    if (!src || !tgt || !corr_out || ns <= 0 || nt <= 0) return r3d_fail(ctx, R3D_E_BADARG, "debug_icp_correspondences: bad argument");
    if (!(max_correspondence_distance > 0)) return r3d_fail(ctx, R3D_E_BADARG, "debug_icp_correspondences: max_correspondence_distance must be > 0");
    R3D_HIP(ctx, hipSetDevice(ctx->device));
    DevArena ar(ctx);
    int rc;
    double *d_t, *d_s;
    if ((rc = upload_pair(ctx, ar, src, ns, tgt, nt, &d_s, &d_t))) return rc;
    r3d_icp_params p = {};
    p.mode = MODE_P2P;
    p.max_correspondence_distance = max_correspondence_distance;
    IcpWork w;
    if ((rc = icp_setup(ctx, ar, &p, {.d_s = d_s, .ns = ns, .d_t = d_t, .nt = nt, .init4x4 = T4x4}, w))) return rc;
    return icp_read_correspondences(ctx, ar, &p, w, d_t, corr_out, d2_out);
}

// diagnostic: what one evaluation of the registration loop accumulates -- icp_core's set-up in the given mode, one k_icp_eval at
// pose T through the loop's own launch, then k_icp_step's reduction of the partial sums
extern "C" int r3d_debug_icp_sums(r3d_ctx *ctx, const r3d_icp_params *p, const double *src, int64_t ns, const double *src_normals,
                                  const double *tgt, int64_t nt, const double *tgt_normals, const double *T4x4, double *sums_out,
                                  double *origin_out) {
    R3D_ROCTX_RANGE("r3d_debug_icp_sums");
    if (!ctx) return R3D_E_BADARG;
    if (!p || !src || !tgt || !sums_out || ns <= 0 || nt <= 0) return r3d_fail(ctx, R3D_E_BADARG, "debug_icp_sums: bad argument");
    int rc;
    if ((rc = icp_mode_check(ctx, "debug_icp_sums", p, tgt_normals != nullptr, src_normals != nullptr))) return rc;
    R3D_HIP(ctx, hipSetDevice(ctx->device));
    DevArena ar(ctx);
    double *d_t, *d_s, *d_tn = nullptr, *d_sn = nullptr;
    if ((rc = upload_pair(ctx, ar, src, ns, tgt, nt, &d_s, &d_t)) || (p->mode != MODE_P2P && (rc = upload(ctx, ar, tgt_normals, nt * 3, &d_tn))) ||
        (p->mode == MODE_GICP && (rc = upload(ctx, ar, src_normals, ns * 3, &d_sn)))) return rc;
    IcpWork w;
    if ((rc = icp_setup(ctx, ar, p, {.d_s = d_s, .ns = ns, .d_sn = d_sn, .d_t = d_t, .nt = nt, .d_tn = d_tn, .init4x4 = T4x4}, w))) return rc;
    return icp_read_sums(ctx, ar, p, w, sums_out, origin_out);
}

// the same read-out for the coloured mode: r3d_icp_colored's checks and set-up, one evaluation, k_icp_step's reduction; and the
// target's records as that set-up computed them
extern "C" int r3d_debug_icp_sums_colored(r3d_ctx *ctx, const r3d_colored_icp_params *p, const double *src, const double *src_colors, int64_t ns,
                                          const double *tgt, const double *tgt_normals, const double *tgt_colors, int64_t nt, const double *T4x4,
                                          double *sums_out, double *tgt_records_out) {
    R3D_ROCTX_RANGE("r3d_debug_icp_sums_colored");
    if (!ctx) return R3D_E_BADARG;
    if (!sums_out) return r3d_fail(ctx, R3D_E_BADARG, "debug_icp_sums_colored: bad argument");
    r3d_icp_params ip;
    IcpColorInput ci;
    int rc;
    // (the check wants a non-null pose argument for the result of the registration calls; here the pose is an optional input)
    if ((rc = colored_icp_check(ctx, "debug_icp_sums_colored", p, src, src_colors, ns, tgt, tgt_normals, tgt_colors, nt, sums_out, &ip, &ci))) return rc;
    R3D_HIP(ctx, hipSetDevice(ctx->device));
    DevArena ar(ctx);
    double *d_t, *d_tn, *d_tc, *d_s, *d_sc;
    if ((rc = upload_pair(ctx, ar, src, ns, tgt, nt, &d_s, &d_t)) || (rc = upload(ctx, ar, tgt_normals, nt * 3, &d_tn)) ||
        (rc = upload(ctx, ar, tgt_colors, nt * 3, &d_tc)) || (rc = upload(ctx, ar, src_colors, ns * 3, &d_sc)))
        return rc;
    ci.d_sc = d_sc; ci.d_tc = d_tc;
    IcpWork w;
    if ((rc = icp_setup(ctx, ar, &ip, {.d_s = d_s, .ns = ns, .d_t = d_t, .nt = nt, .d_tn = d_tn, .init4x4 = T4x4, .color = &ci}, w))) return rc;
    if ((rc = r3d_download(ctx, tgt_records_out, w.d_trec, (size_t)nt * 4))) return rc;
    return icp_read_sums(ctx, ar, &ip, w, sums_out, nullptr);   // synchronises the stream
}

extern "C" int r3d_debug_exclusive_scan(r3d_ctx *ctx, const int32_t *in, int64_t n, int32_t op, int32_t *out) {
    R3D_ROCTX_RANGE("r3d_debug_exclusive_scan");
    if (!ctx) return R3D_E_BADARG;
    if (!in || !out || n <= 0 || op < 0 || op > 1) return r3d_fail(ctx, R3D_E_BADARG, "debug_exclusive_scan: bad argument");
    R3D_HIP(ctx, hipSetDevice(ctx->device));
    DevArena ar(ctx);
    const int *d_in;
    if (int rc = r3d_upload(ctx, ar, in, (size_t)n, &d_in)) return rc;
    int *d_out = (int *)ar.get((size_t)n * 4);
    if (ar.rc) return ar.rc;
    int rc = op == 1 ? dev_exclusive_scan<int, true>(ctx, ar, d_in, d_out, n) : dev_exclusive_scan<int>(ctx, ar, d_in, d_out, n);
    if (rc || (rc = r3d_download(ctx, out, d_out, (size_t)n))) return rc;
    R3D_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return R3D_OK;
}
