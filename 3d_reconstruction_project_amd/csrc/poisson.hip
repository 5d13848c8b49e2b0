// Screened Poisson surface reconstruction on a dense 2^depth grid ("Poisson reconstruction"; C ABI:
// r3d_poisson_*).  Everything is float64 and every sum has a fixed order (-ffp-contract=off), so the fields are bit for bit those of
// tests/poisson_ref.py.  Node (i, j, k) of the G = 2^depth + 1 nodes per axis lies at (k G + j) G + i; vector fields are one plane
// per component.  The stages:
//   ordering    the points in the stable order of their cell (cloud.hip's cell sort), the first point of every cell, and every
//               point's fractions inside its cell;
//   splats      two gathers, one thread per node over its eight cells and their points in ascending point number (no float
//               atomics), with the density pass between them;
//   solve       divergence, then V-cycles of weighted Jacobi with full-weighting restriction and trilinear prolongation;
//   extraction  marching cubes at iso 0 in four steps: cube bytes, counts, scans, then vertices and triangles.
// No kernel waits on another workgroup; every buffer comes from the context's arena.
#include <algorithm>
#include <cstring>

#include "r3d_internal.h"
#include "tsdf_mc_tables.h"

namespace {

struct PoGrid {
    int R, G;            // cells and nodes per axis
    double org[3], h;
};

// ---- bounds and the finiteness test ----------------------------------------------------------------------------------------------------
// part[b][0..2] = min, [3..5] = max of the finite coordinates seen by block b, [6] = how many non-finite coordinates or normal
// components it saw; k_po_bounds_final folds the rows into row 0 (minima and maxima are exact, so the order does not matter)
constexpr int PO_BOUNDS_BLOCKS = 256;
__device__ __forceinline__ void po_fold7(double (*sm)[256], int tid) {
    for (int off = 128; off > 0; off >>= 1) {
        __syncthreads();
        if (tid < off) {
            for (int a = 0; a < 3; a++) {
                sm[a][tid] = fmin(sm[a][tid], sm[a][tid + off]);
                sm[3 + a][tid] = fmax(sm[3 + a][tid], sm[3 + a][tid + off]);
            }
            sm[6][tid] += sm[6][tid + off];
        }
    }
    __syncthreads();
}
__global__ void __launch_bounds__(256) k_po_bounds(const double *__restrict__ p, const double *__restrict__ nrm, int n, double *__restrict__ part) {
    __shared__ double sm[7][256];
    const int tid = (int)threadIdx.x;
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY}, bad = 0.0;
    for (int64_t e = (int64_t)blockIdx.x * 256 + tid; e < (int64_t)n * 3; e += (int64_t)gridDim.x * 256) {
        const double x = p[e];
        const int a = (int)(e % 3);
        if (!isfinite(x) || !isfinite(nrm[e])) bad += 1.0;
#pragma unroll
        for (int c = 0; c < 3; c++)
            if (c == a && isfinite(x)) { lo[c] = fmin(lo[c], x); hi[c] = fmax(hi[c], x); }
    }
    for (int a = 0; a < 3; a++) { sm[a][tid] = lo[a]; sm[3 + a][tid] = hi[a]; }
    sm[6][tid] = bad;
    po_fold7(sm, tid);
    if (tid < 7) part[blockIdx.x * 7 + tid] = sm[tid][0];
}
__global__ void __launch_bounds__(256) k_po_bounds_final(double *__restrict__ part, int rows) {
    __shared__ double sm[7][256];
    const int tid = (int)threadIdx.x;
    for (int a = 0; a < 7; a++) sm[a][tid] = tid < rows ? part[tid * 7 + a] : (a < 3 ? INFINITY : a < 6 ? -INFINITY : 0.0);
    po_fold7(sm, tid);
    if (tid < 7) part[tid] = sm[tid][0];
}

// ---- ordering --------------------------------------------------------------------------------------------------------------------------
// keys are sorted: first[key] = the position of the first point of cell `key` (the table is preset to -1)
__global__ void __launch_bounds__(256) k_po_cell_first(const unsigned *__restrict__ keys, int n, int *__restrict__ first) {
    const int q = (int)(blockIdx.x * 256 + threadIdx.x);
    if (q >= n) return;
    const unsigned key = keys[q];
    if (q == 0 || keys[q - 1] != key) first[key] = q;
}
__device__ __forceinline__ void po_cell_of(unsigned key, int R, int c[3]) {
    c[2] = (int)(key % (unsigned)R);
    c[1] = (int)((key / (unsigned)R) % (unsigned)R);
    c[0] = (int)(key / ((unsigned)R * (unsigned)R));
}
// frac[q][a] = g - cell, g = (p - org) / h: a division, as the sort's key has it
__global__ void __launch_bounds__(256) k_po_fractions(PoGrid g, const double *__restrict__ p, const unsigned *__restrict__ keys,
                                                      const int *__restrict__ idx, int n, double *__restrict__ frac) {
    const int q = (int)(blockIdx.x * 256 + threadIdx.x);
    if (q >= n) return;
    int c[3];
    po_cell_of(keys[q], g.R, c);
    const size_t i = (size_t)idx[q];
    for (int a = 0; a < 3; a++) frac[(size_t)q * 3 + a] = (p[i * 3 + a] - g.org[a]) / g.h - (double)c[a];
}

// ---- splats ----------------------------------------------------------------------------------------------------------------------------
// One thread per node: the eight incident cells in the order of their offset (dz, dy, dx) from (-1,-1,-1) to (0,0,0), the points
// of a cell in ascending number (the sort is stable).  PASS 1: s0 = W0 and, with attr = the colours, s3 = C0.  PASS 2: the weight
// carries wt = 1 / density; s0 = D, s3 = V with attr = the normals.
template <int PASS>
__global__ void __launch_bounds__(256) k_po_gather(PoGrid g, int n, const int *__restrict__ first, const unsigned *__restrict__ keys,
                                                   const int *__restrict__ idx, const double *__restrict__ frac, const double *__restrict__ attr,
                                                   const double *__restrict__ wt_s, double *__restrict__ s0, double *__restrict__ s3) {
    const int G = g.G, R = g.R;
    const size_t G3 = (size_t)G * G * G, t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= G3) return;
    const int i = (int)(t % G), j = (int)((t / G) % G), k = (int)(t / ((size_t)G * G));
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    for (int dz = -1; dz <= 0; dz++)
        for (int dy = -1; dy <= 0; dy++)
            for (int dx = -1; dx <= 0; dx++) {
                const int cx = i + dx, cy = j + dy, cz = k + dz;
                if (cx < 0 || cy < 0 || cz < 0 || cx >= R || cy >= R || cz >= R) continue;
                const unsigned key = ((unsigned)cx * R + cy) * R + cz;
                int q = first[key];
                if (q < 0) continue;
                for (; q < n && keys[q] == key; q++) {
                    const double fx = frac[(size_t)q * 3], fy = frac[(size_t)q * 3 + 1], fz = frac[(size_t)q * 3 + 2];
                    const double wx = dx ? fx : 1.0 - fx, wy = dy ? fy : 1.0 - fy, wz = dz ? fz : 1.0 - fz;   // the node is corner -d of the cell
                    double w = (wx * wy) * wz;
                    if (PASS == 2) w = w * wt_s[q];
                    a0 += w;
                    if (attr) {
                        const size_t pi = (size_t)idx[q] * 3;
                        a1 += w * attr[pi]; a2 += w * attr[pi + 1]; a3 += w * attr[pi + 2];
                    }
                }
            }
    s0[t] = a0;
    if (attr) { s3[t] = a1; s3[G3 + t] = a2; s3[2 * G3 + t] = a3; }
}
// dens = the trilinear interpolation of W0 at the point, corners in the order dz, dy, dx; dens[point] and wt_s[position] = 1 / dens
__global__ void __launch_bounds__(256) k_po_density(PoGrid g, int n, const unsigned *__restrict__ keys, const int *__restrict__ idx,
                                                    const double *__restrict__ frac, const double *__restrict__ W0, double *__restrict__ dens,
                                                    double *__restrict__ wt_s) {
    const int q = (int)(blockIdx.x * 256 + threadIdx.x);
    if (q >= n) return;
    int c[3];
    po_cell_of(keys[q], g.R, c);
    const int G = g.G;
    const size_t base = ((size_t)c[2] * G + c[1]) * G + c[0];
    const double fx = frac[(size_t)q * 3], fy = frac[(size_t)q * 3 + 1], fz = frac[(size_t)q * 3 + 2];
    double d = 0.0;
    for (int dz = 0; dz < 2; dz++)
        for (int dy = 0; dy < 2; dy++)
            for (int dx = 0; dx < 2; dx++) {
                const double wx = dx ? fx : 1.0 - fx, wy = dy ? fy : 1.0 - fy, wz = dz ? fz : 1.0 - fz;
                d += ((wx * wy) * wz) * W0[base + ((size_t)dz * G + dy) * G + dx];
            }
    dens[idx[q]] = d;
    wt_s[q] = 1.0 / d;
}

// ---- right-hand side -------------------------------------------------------------------------------------------------------------------
// b = -1/2 [(Vx(i+1) - Vx(i-1)) + (Vy(j+1) - Vy(j-1)) + (Vz(k+1) - Vz(k-1))], V = 0 outside the grid; diag = alpha D
__global__ void __launch_bounds__(256) k_po_divergence(int G, const double *__restrict__ V, const double *__restrict__ D, double alpha,
                                                       double *__restrict__ b, double *__restrict__ diag) {
    const size_t G2 = (size_t)G * G, G3 = G2 * G, t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= G3) return;
    const int i = (int)(t % G), j = (int)((t / G) % G), k = (int)(t / G2);
    const double *Vx = V, *Vy = V + G3, *Vz = V + 2 * G3;
    const double xp = i + 1 < G ? Vx[t + 1] : 0.0, xm = i > 0 ? Vx[t - 1] : 0.0;
    const double yp = j + 1 < G ? Vy[t + G] : 0.0, ym = j > 0 ? Vy[t - G] : 0.0;
    const double zp = k + 1 < G ? Vz[t + G2] : 0.0, zm = k > 0 ? Vz[t - G2] : 0.0;
    b[t] = -0.5 * (((xp - xm) + (yp - ym)) + (zp - zm));
    diag[t] = alpha * D[t];
}

// ---- solver ----------------------------------------------------------------------------------------------------------------------------
// The sum of the six neighbours in the contract's order
__device__ __forceinline__ double po_six(const double *__restrict__ x, size_t t, int G, size_t G2) {
    return ((((x[t + 1] + x[t - 1]) + x[t + G]) + x[t - G]) + x[t + G2]) + x[t - G2];
}
// One weighted-Jacobi sweep in -> out over the interior nodes: out = x + omega ((b + s) / (6 + diag) - x).  A thread owns an (i, j)
// column of PO_ZC planes and keeps the plane below, its own and the one above in registers; lanes run along x.
constexpr int PO_ZC = 8;
__global__ void __launch_bounds__(256) k_po_jacobi(int G, const double *__restrict__ in, double *__restrict__ out, const double *__restrict__ b,
                                                   const double *__restrict__ diag, double omega) {
    const int i = 1 + (int)(blockIdx.x * 64 + threadIdx.x), j = 1 + (int)(blockIdx.y * 4 + threadIdx.y);
    if (i > G - 2 || j > G - 2) return;
    const int k0 = 1 + (int)blockIdx.z * PO_ZC, k1 = min(k0 + PO_ZC, G - 1);
    const size_t G2 = (size_t)G * G;
    size_t t = (size_t)k0 * G2 + (size_t)j * G + i;
    double lo = in[t - G2], c = in[t];
    for (int k = k0; k < k1; k++, t += G2) {
        const double hi = in[t + G2];
        const double s = ((((in[t + 1] + in[t - 1]) + in[t + G]) + in[t - G]) + hi) + lo;
        out[t] = c + omega * ((b[t] + s) / (6.0 + diag[t]) - c);
        lo = c;
        c = hi;
    }
}
// The coarsest level (G <= 5) in one workgroup: `sweeps` sweeps between two LDS copies, the result back into x
__global__ void __launch_bounds__(128) k_po_coarsest(int G, double *__restrict__ x, const double *__restrict__ b, const double *__restrict__ diag,
                                                     double omega, int sweeps) {
    __shared__ double u[2][125];
    const int t = (int)threadIdx.x, G2 = G * G, G3 = G2 * G;
    const int i = t % G, j = (t / G) % G, k = t / G2;
    const bool live = t < G3, inner = live && i > 0 && j > 0 && k > 0 && i < G - 1 && j < G - 1 && k < G - 1;
    if (live) u[0][t] = u[1][t] = x[t];
    const double bb = inner ? b[t] : 0.0, den = inner ? 6.0 + diag[t] : 1.0;
    __syncthreads();
    int cur = 0;
    for (int s = 0; s < sweeps; s++, cur ^= 1) {
        if (inner) {
            const double *v = u[cur];
            const double six = ((((v[t + 1] + v[t - 1]) + v[t + G]) + v[t - G]) + v[t + G2]) + v[t - G2];
            u[cur ^ 1][t] = v[t] + omega * ((bb + six) / den - v[t]);
        }
        __syncthreads();
    }
    if (inner) x[t] = u[cur][t];
}
// Full weighting of a fine field onto the interior nodes of the coarse grid, as three one-axis passes x, y, z of
// (0.25 a + 0.5 b) + 0.25 c with the coarse node I at the fine node 2 I, times 4.  RESIDUAL: the field is r = b - A x, computed on
// the fly; else it is `f` itself.  An interior coarse node reads interior fine nodes only.
template <bool RESIDUAL>
__global__ void __launch_bounds__(256) k_po_restrict(int Gf, int Gc, const double *__restrict__ f, const double *__restrict__ x,
                                                     const double *__restrict__ diag, double *__restrict__ out) {
    const int n1 = Gc - 2;
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (size_t)n1 * n1 * n1) return;
    const int I = 1 + (int)(t % n1), J = 1 + (int)((t / n1) % n1), K = 1 + (int)(t / ((size_t)n1 * n1));
    const size_t F2 = (size_t)Gf * Gf;
    double pz[3];
#pragma unroll
    for (int dz = 0; dz < 3; dz++) {
        double py[3];
#pragma unroll
        for (int dy = 0; dy < 3; dy++) {
            double px[3];
#pragma unroll
            for (int dx = 0; dx < 3; dx++) {
                const size_t e = (size_t)(2 * K + dz - 1) * F2 + (size_t)(2 * J + dy - 1) * Gf + (size_t)(2 * I + dx - 1);
                if (RESIDUAL) {
                    const double c = x[e];
                    px[dx] = f[e] - ((6.0 * c - po_six(x, e, Gf, F2)) + diag[e] * c);
                } else {
                    px[dx] = f[e];
                }
            }
            py[dy] = (0.25 * px[0] + 0.5 * px[1]) + 0.25 * px[2];
        }
        pz[dz] = (0.25 * py[0] + 0.5 * py[1]) + 0.25 * py[2];
    }
    out[((size_t)K * Gc + J) * Gc + I] = 4.0 * ((0.25 * pz[0] + 0.5 * pz[1]) + 0.25 * pz[2]);
}
// x += the trilinear prolongation of the coarse e, as three one-axis passes x, y, z: an even node takes the coarse value, an odd one
// 0.5 (a + b); interior fine nodes only
__global__ void __launch_bounds__(256) k_po_prolong_add(int Gf, int Gc, const double *__restrict__ e, double *__restrict__ x) {
    const int n1 = Gf - 2;
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (size_t)n1 * n1 * n1) return;
    const int i = 1 + (int)(t % n1), j = 1 + (int)((t / n1) % n1), k = 1 + (int)(t / ((size_t)n1 * n1));
    const size_t C2 = (size_t)Gc * Gc;
    auto px = [&](int J, int K) {
        const double *row = e + (size_t)K * C2 + (size_t)J * Gc;
        return (i & 1) ? 0.5 * (row[i >> 1] + row[(i >> 1) + 1]) : row[i >> 1];
    };
    auto py = [&](int K) { return (j & 1) ? 0.5 * (px(j >> 1, K) + px((j >> 1) + 1, K)) : px(j >> 1, K); };
    const double v = (k & 1) ? 0.5 * (py(k >> 1) + py((k >> 1) + 1)) : py(k >> 1);
    const size_t o = ((size_t)k * Gf + j) * Gf + i;
    x[o] = x[o] + v;
}

// ---- extraction ------------------------------------------------------------------------------------------------------------------------
// Marching cubes at iso 0 with the TSDF mesh's table, sign rule (inside iff chi < 0) and winding.  A vertex is owned by (lower node
// of its edge, axis): vertices in node order then axis, triangles in base-node order then the table's.
__device__ const int8_t d_po_tri[256][16] = TSDF_MC_TRI_ROWS;
__device__ const uint8_t d_po_count[256] = TSDF_MC_COUNT_ROWS;
constexpr unsigned long long po_edge_pack() {
    unsigned long long p = 0;
    for (int e = 0; e < 12; e++) p |= (unsigned long long)TSDF_MC_EDGE[e] << (5 * e);
    return p;
}
constexpr unsigned long long PO_EDGE_PACK = po_edge_pack();

// the cube byte of every node: bit c = corner c inside, for the base nodes of the R^3 cubes; 0 on the top faces
__global__ void __launch_bounds__(256) k_po_mc_cubes(int G, const double *__restrict__ chi, uint8_t *__restrict__ cube) {
    const size_t G2 = (size_t)G * G, G3 = G2 * G, t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= G3) return;
    const int i = (int)(t % G), j = (int)((t / G) % G), k = (int)(t / G2);
    unsigned B = 0;
    if (i < G - 1 && j < G - 1 && k < G - 1) {
#pragma unroll
        for (int c = 0; c < 8; c++) {
            const size_t e = t + (size_t)(c >> 2) * G2 + (size_t)((c >> 1) & 1) * G + (size_t)(((c + 1) >> 1) & 1);
            B |= (chi[e] < 0.0 ? 1u : 0u) << c;
        }
    }
    cube[t] = (uint8_t)B;
}
// per node: which of its three edges carry a vertex (bit a = axis a), how many, and the triangles of its cube
__global__ void __launch_bounds__(256) k_po_mc_count(int G, const double *__restrict__ chi, const uint8_t *__restrict__ cube,
                                                     uint8_t *__restrict__ emask, int *__restrict__ cntv, int *__restrict__ cntt) {
    const size_t G2 = (size_t)G * G, G3 = G2 * G, t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= G3) return;
    const int i = (int)(t % G), j = (int)((t / G) % G), k = (int)(t / G2);
    const bool in0 = chi[t] < 0.0;
    unsigned m = 0;
    if (i < G - 1 && (chi[t + 1] < 0.0) != in0) m |= 1u;
    if (j < G - 1 && (chi[t + G] < 0.0) != in0) m |= 2u;
    if (k < G - 1 && (chi[t + G2] < 0.0) != in0) m |= 4u;
    emask[t] = (uint8_t)m;
    cntv[t] = __popc(m);
    cntt[t] = d_po_count[cube[t]];
}
// t = chi_a / (chi_a - chi_b); the coordinate on the edge axis is org + h (i + t); density and colour interpolate W0 and C0
__global__ void __launch_bounds__(256) k_po_mc_vertices(PoGrid g, const double *__restrict__ chi, const double *__restrict__ W0,
                                                        const double *__restrict__ C0, const uint8_t *__restrict__ emask,
                                                        const int *__restrict__ offv, double *__restrict__ vert, double *__restrict__ dens,
                                                        double *__restrict__ col) {
    const int G = g.G;
    const size_t G2 = (size_t)G * G, G3 = G2 * G, t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= G3) return;
    const unsigned m = emask[t];
    if (!m) return;
    const int c[3] = {(int)(t % G), (int)((t / G) % G), (int)(t / G2)};
    const size_t stride[3] = {1, (size_t)G, G2};
    size_t o = (size_t)offv[t];
    const double ca = chi[t], wa = W0[t];
    for (int a = 0; a < 3; a++) {
        if (!((m >> a) & 1u)) continue;
        const size_t u = t + stride[a];
        const double cb = chi[u], tt = ca / (ca - cb);
        for (int d = 0; d < 3; d++) vert[o * 3 + d] = d == a ? g.org[d] + g.h * ((double)c[d] + tt) : g.org[d] + g.h * (double)c[d];
        const double de = (1.0 - tt) * wa + tt * W0[u];
        dens[o] = de;
        if (col)
            for (int ch = 0; ch < 3; ch++)
                col[o * 3 + ch] = de != 0.0 ? ((1.0 - tt) * C0[ch * G3 + t] + tt * C0[ch * G3 + u]) / de : 0.0;
        o++;
    }
}
__global__ void __launch_bounds__(256) k_po_mc_triangles(int G, const uint8_t *__restrict__ cube, const uint8_t *__restrict__ emask,
                                                         const int *__restrict__ offv, const int *__restrict__ offt, int32_t *__restrict__ tri) {
    const size_t G2 = (size_t)G * G, G3 = G2 * G, t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= G3) return;
    const unsigned B = cube[t];
    const int n = d_po_count[B];
    size_t o = (size_t)offt[t];
    for (int q = 0; q < n; q++, o++) {
        int32_t id[3];
        for (int v = 0; v < 3; v++) {
            const unsigned code = (unsigned)(PO_EDGE_PACK >> (5 * d_po_tri[B][3 * q + v])) & 31u;
            const size_t lower = t + (size_t)(code & 1u) + (size_t)((code >> 1) & 1u) * G + (size_t)((code >> 2) & 1u) * G2;
            const unsigned axis = code >> 3;
            id[v] = offv[lower] + __popc((unsigned)emask[lower] & ((1u << axis) - 1u));
        }
        tri[o * 3] = id[0]; tri[o * 3 + 1] = id[2]; tri[o * 3 + 2] = id[1];
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------------------------
constexpr r3d_poisson_params PO_DEFAULTS = {8, 10, 2, 2, 40, 0, 1.1, 4.0, 0.8};

int po_params_ok(r3d_ctx *ctx, const r3d_poisson_params &p) {
    if (p.cycles < 0 || p.pre < 0 || p.post < 0 || p.coarse_sweeps < 0 || !(p.scale > 0.0) || !std::isfinite(p.scale) || !(p.alpha >= 0.0) ||
        !std::isfinite(p.alpha) || !(p.omega > 0.0) || !std::isfinite(p.omega))
        return r3d_fail(ctx, R3D_E_BADARG, "poisson: a negative count, or scale, alpha or omega out of range");
    if (p.depth < 2 || p.depth > 8) return r3d_fail(ctx, R3D_E_UNSUPPORTED, "poisson: depth %d is outside 2..8 (the grid is dense)", p.depth);
    return R3D_OK;
}

// the fields of one reconstruction, in arena buffers
struct PoFields {
    PoGrid g = {};
    size_t G3 = 0;
    double *W0 = nullptr, *C0 = nullptr, *dens = nullptr, *V = nullptr, *D = nullptr, *b = nullptr, *diag = nullptr, *chi = nullptr;
};
struct PoLevel { int G; double *x, *y, *rhs, *diag; };   // x: the current iterate, y: the other buffer of the ping-pong

int po_sweeps(r3d_ctx *ctx, PoLevel &L, int count, double omega) {
    const int m = L.G - 2;
    const dim3 grid((unsigned)((m + 63) / 64), (unsigned)((m + 3) / 4), (unsigned)((m + PO_ZC - 1) / PO_ZC));
    for (int s = 0; s < count; s++) {
        k_po_jacobi<<<grid, dim3(64, 4, 1), 0, ctx->stream>>>(L.G, L.x, L.y, L.rhs, L.diag, omega);
        std::swap(L.x, L.y);
    }
    R3D_HIP(ctx, hipGetLastError());
    return R3D_OK;
}
int po_vcycle(r3d_ctx *ctx, std::vector<PoLevel> &lv, size_t l, const r3d_poisson_params &p) {
    PoLevel &L = lv[l];
    if (L.G <= 5) {
        k_po_coarsest<<<1, 128, 0, ctx->stream>>>(L.G, L.x, L.rhs, L.diag, p.omega, p.coarse_sweeps);
        R3D_HIP(ctx, hipGetLastError());
        return R3D_OK;
    }
    PoLevel &C = lv[l + 1];
    int rc;
    if ((rc = po_sweeps(ctx, L, p.pre, p.omega))) return rc;
    const size_t nc = (size_t)(C.G - 2) * (C.G - 2) * (C.G - 2), nf = (size_t)(L.G - 2) * (L.G - 2) * (L.G - 2);
    k_po_restrict<true><<<r3d_blocks(nc), 256, 0, ctx->stream>>>(L.G, C.G, L.rhs, L.x, L.diag, C.rhs);
    R3D_HIP(ctx, hipMemsetAsync(C.x, 0, (size_t)C.G * C.G * C.G * 8, ctx->stream));
    if ((rc = po_vcycle(ctx, lv, l + 1, p))) return rc;
    k_po_prolong_add<<<r3d_blocks(nf), 256, 0, ctx->stream>>>(L.G, C.G, C.x, L.x);
    R3D_HIP(ctx, hipGetLastError());
    return po_sweeps(ctx, L, p.post, p.omega);
}

// bounds, ordering, splats, right-hand side and `cycles` V-cycles from chi = 0; enqueues after the one read-back of the bounds
int po_solve(r3d_ctx *ctx, DevArena &ar, const double *d_xyz, const double *d_nrm, const double *d_col, int64_t n64, const r3d_poisson_params &p,
             int cycles, PoFields &F) {
    hipStream_t st = ctx->stream;
    const int n = (int)n64;
    r3d_prof_begin(ctx, ctx->ws[0]);   // stage times for tools/gpu_bench_poisson.py when the context profiles (r3d_set_profiling)
    r3d_prof_mark(ctx, ctx->ws[0], st, "poisson_ordering");
    // grid
    double *part = (double *)ar.get((size_t)PO_BOUNDS_BLOCKS * 7 * 8);
    if (ar.rc) return ar.rc;
    const int bb = (int)std::min<int64_t>(PO_BOUNDS_BLOCKS, ((int64_t)n * 3 + 255) / 256);
    k_po_bounds<<<bb, 256, 0, st>>>(d_xyz, d_nrm, n, part);
    k_po_bounds_final<<<1, 256, 0, st>>>(part, bb);
    R3D_HIP(ctx, hipGetLastError());
    double h7[7];
    R3D_HIP(ctx, hipMemcpyAsync(h7, part, sizeof(h7), hipMemcpyDeviceToHost, st));
    R3D_HIP(ctx, hipStreamSynchronize(st));
    if (h7[6] != 0.0) return r3d_fail(ctx, R3D_E_BADARG, "poisson: %.0f non-finite coordinates or normal components", h7[6]);
    double ext = 0.0;
    for (int a = 0; a < 3; a++) ext = std::max(ext, h7[3 + a] - h7[a]);
    const double s = p.scale * ext;
    if (!(s > 0.0) || !std::isfinite(s)) return r3d_fail(ctx, R3D_E_BADARG, "poisson: the points span a cube of side %g", s);
    PoGrid &g = F.g;
    g.R = 1 << p.depth;
    g.G = g.R + 1;
    g.h = s / (double)g.R;
    for (int a = 0; a < 3; a++) g.org[a] = (h7[a] + h7[3 + a]) / 2.0 - s / 2.0;
    const int G = g.G, R = g.R;
    const size_t G3 = F.G3 = (size_t)G * G * G, R3 = (size_t)R * R * R;

    // ordering
    const unsigned *keys = nullptr;
    const int *idx = nullptr;
    const int dims[3] = {R, R, R};
    int rc;
    if ((rc = r3d_sort_by_voxel_u32(ctx, ar, d_xyz, n, g.org, g.h, dims, &keys, &idx))) return rc;
    int *first = (int *)ar.get(R3 * 4);
    double *frac = (double *)ar.get((size_t)n * 3 * 8), *wt_s = (double *)ar.get((size_t)n * 8);
    F.W0 = (double *)ar.get(G3 * 8);
    F.C0 = d_col ? (double *)ar.get(G3 * 3 * 8) : nullptr;
    F.dens = (double *)ar.get((size_t)n * 8);
    F.V = (double *)ar.get(G3 * 3 * 8);
    F.D = (double *)ar.get(G3 * 8);
    F.b = (double *)ar.get(G3 * 8);
    F.diag = (double *)ar.get(G3 * 8);
    std::vector<PoLevel> lv;
    for (int Gl = G;; Gl = (Gl - 1) / 2 + 1) {
        const size_t bytes = (size_t)Gl * Gl * Gl * 8;
        PoLevel L = {Gl, (double *)ar.get(bytes), (double *)ar.get(bytes), nullptr, nullptr};
        L.rhs = lv.empty() ? F.b : (double *)ar.get(bytes);
        L.diag = lv.empty() ? F.diag : (double *)ar.get(bytes);
        lv.push_back(L);
        if (Gl <= 5) break;
    }
    if (ar.rc) return ar.rc;
    R3D_HIP(ctx, hipMemsetAsync(first, 0xFF, R3 * 4, st));
    k_po_cell_first<<<r3d_blocks((size_t)n), 256, 0, st>>>(keys, n, first);
    k_po_fractions<<<r3d_blocks((size_t)n), 256, 0, st>>>(g, d_xyz, keys, idx, n, frac);

    // splats
    r3d_prof_mark(ctx, ctx->ws[0], st, "poisson_splats");
    k_po_gather<1><<<r3d_blocks(G3), 256, 0, st>>>(g, n, first, keys, idx, frac, d_col, nullptr, F.W0, F.C0);
    k_po_density<<<r3d_blocks((size_t)n), 256, 0, st>>>(g, n, keys, idx, frac, F.W0, F.dens, wt_s);
    k_po_gather<2><<<r3d_blocks(G3), 256, 0, st>>>(g, n, first, keys, idx, frac, d_nrm, wt_s, F.D, F.V);

    // solve: right-hand side, the coarse diagonals, then the cycles.  Both buffers of every level start at zero and a sweep writes
    // interior nodes only, so the faces stay zero.
    r3d_prof_mark(ctx, ctx->ws[0], st, "poisson_solve");
    k_po_divergence<<<r3d_blocks(G3), 256, 0, st>>>(G, F.V, F.D, p.alpha, F.b, F.diag);
    R3D_HIP(ctx, hipGetLastError());
    for (size_t l = 0; l < lv.size(); l++) {
        const size_t bytes = (size_t)lv[l].G * lv[l].G * lv[l].G * 8;
        R3D_HIP(ctx, hipMemsetAsync(lv[l].x, 0, bytes, st));
        R3D_HIP(ctx, hipMemsetAsync(lv[l].y, 0, bytes, st));
        if (l) {
            const size_t nc = (size_t)(lv[l].G - 2) * (lv[l].G - 2) * (lv[l].G - 2);
            R3D_HIP(ctx, hipMemsetAsync(lv[l].diag, 0, bytes, st));
            R3D_HIP(ctx, hipMemsetAsync(lv[l].rhs, 0, bytes, st));
            k_po_restrict<false><<<r3d_blocks(nc), 256, 0, st>>>(lv[l - 1].G, lv[l].G, lv[l - 1].diag, nullptr, nullptr, lv[l].diag);
        }
    }
    R3D_HIP(ctx, hipGetLastError());
    for (int c = 0; c < cycles; c++)
        if ((rc = po_vcycle(ctx, lv, 0, p))) return rc;
    F.chi = lv[0].x;
    r3d_prof_mark(ctx, ctx->ws[0], st, "poisson_extraction");   // closed by the caller's r3d_prof_end, after its extraction if it has one
    return R3D_OK;
}

// the extraction in two halves, as the TSDF mesh's: counts (always), then vertices and triangles into device arrays
struct PoMeshWork {
    PoGrid g = {};
    const double *chi = nullptr, *W0 = nullptr, *C0 = nullptr;
    uint8_t *cube = nullptr, *emask = nullptr;
    int *offv = nullptr, *offt = nullptr;
    long long total[2] = {0, 0};
};
int po_mesh_count(r3d_ctx *ctx, DevArena &ar, PoMeshWork &W, int64_t *out_nv, int64_t *out_nt) {
    hipStream_t st = ctx->stream;
    const int G = W.g.G;
    const size_t G3 = (size_t)G * G * G;
    W.cube = (uint8_t *)ar.get(G3);
    W.emask = (uint8_t *)ar.get(G3);
    int *cntv = (int *)ar.get(G3 * 4), *cntt = (int *)ar.get(G3 * 4);
    W.offv = (int *)ar.get(G3 * 4);
    W.offt = (int *)ar.get(G3 * 4);
    if (ar.rc) return ar.rc;
    k_po_mc_cubes<<<r3d_blocks(G3), 256, 0, st>>>(G, W.chi, W.cube);
    k_po_mc_count<<<r3d_blocks(G3), 256, 0, st>>>(G, W.chi, W.cube, W.emask, cntv, cntt);
    R3D_HIP(ctx, hipGetLastError());
    int rc;
    if ((rc = r3d_exclusive_scan_i32(ctx, ar, cntv, W.offv, (int64_t)G3)) || (rc = r3d_exclusive_scan_i32(ctx, ar, cntt, W.offt, (int64_t)G3))) return rc;
    int last[4];
    if ((rc = r3d_read_back(ctx, {{&last[0], W.offv + G3 - 1, 4}, {&last[1], cntv + G3 - 1, 4}, {&last[2], W.offt + G3 - 1, 4}, {&last[3], cntt + G3 - 1, 4}})))
        return rc;
    *out_nv = W.total[0] = (long long)last[0] + last[1];
    *out_nt = W.total[1] = (long long)last[2] + last[3];
    return R3D_OK;
}
int po_mesh_emit(r3d_ctx *ctx, const PoMeshWork &W, double *d_vert, double *d_dens, double *d_col, int32_t *d_tri) {
    const int G = W.g.G;
    const size_t G3 = (size_t)G * G * G;
    k_po_mc_vertices<<<r3d_blocks(G3), 256, 0, ctx->stream>>>(W.g, W.chi, W.W0, W.C0, W.emask, W.offv, d_vert, d_dens, W.C0 ? d_col : nullptr);
    k_po_mc_triangles<<<r3d_blocks(G3), 256, 0, ctx->stream>>>(G, W.cube, W.emask, W.offv, W.offt, d_tri);
    R3D_HIP(ctx, hipGetLastError());
    return R3D_OK;
}

int po_out_args_ok(r3d_ctx *ctx, const char *who, bool color, int64_t cap_v, int64_t cap_t, const void *vert, const void *dens, const void *col,
                   const void *tri, const void *out_nv, const void *out_nt) {
    if (!out_nv || !out_nt || cap_v < 0 || cap_t < 0 || (cap_v > 0 && (!vert || !dens || (color && !col))) || (cap_t > 0 && !tri))
        return r3d_fail(ctx, R3D_E_BADARG, "%s: a missing array or a negative capacity", who);
    return R3D_OK;
}
int po_in_args_ok(r3d_ctx *ctx, const char *who, const double *xyz, const double *nrm, int64_t n, const r3d_poisson_params *params,
                  r3d_poisson_params &p) {
    if (!xyz || !nrm || n <= 0 || n > INT32_MAX / 4) return r3d_fail(ctx, R3D_E_BADARG, "%s: no points, no normals, or more than 2^29 points", who);
    p = params ? *params : PO_DEFAULTS;
    return po_params_ok(ctx, p);
}
// `both empty`: nothing to write; else the refusal of a capacity that is too small
int po_fits(r3d_ctx *ctx, const char *who, const PoMeshWork &W, int64_t cap_v, int64_t cap_t) {
    if (int rc = r3d_fits(ctx, who, "vertices", W.total[0], cap_v)) return rc;
    return r3d_fits(ctx, who, "triangles", W.total[1], cap_t);
}

// the shared tail of the host-buffer forms: count, refuse or emit into arena arrays, copy out, synchronise
int po_mesh_to_host(r3d_ctx *ctx, DevArena &ar, const char *who, PoMeshWork &W, int64_t cap_v, int64_t cap_t, double *vert, double *dens, double *col,
                    int32_t *tri, int64_t *out_nv, int64_t *out_nt) {
    int rc;
    if ((rc = po_mesh_count(ctx, ar, W, out_nv, out_nt))) return rc;
    if ((cap_v == 0 && cap_t == 0) || (W.total[0] == 0 && W.total[1] == 0)) return R3D_OK;
    if ((rc = po_fits(ctx, who, W, cap_v, cap_t))) return rc;
    const size_t nv = (size_t)W.total[0], nt = (size_t)W.total[1];
    double *d_vert = (double *)ar.get(nv * 3 * 8), *d_dens = (double *)ar.get(nv * 8), *d_col = W.C0 ? (double *)ar.get(nv * 3 * 8) : nullptr;
    int32_t *d_tri = (int32_t *)ar.get(nt * 3 * 4);
    if (ar.rc) return ar.rc;
    if ((rc = po_mesh_emit(ctx, W, d_vert, d_dens, d_col, d_tri)) || (rc = r3d_download(ctx, vert, d_vert, nv * 3)) ||
        (rc = r3d_download(ctx, dens, d_dens, nv)) || (rc = r3d_download(ctx, col, d_col, d_col ? nv * 3 : 0)) ||
        (rc = r3d_download(ctx, tri, d_tri, nt * 3)))
        return rc;
    r3d_prof_end(ctx, ctx->ws[0], ctx->stream);
    R3D_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return R3D_OK;
}

}  // namespace

extern "C" {

int r3d_poisson_reconstruct(r3d_ctx *ctx, const double *xyz, const double *normals, const double *colors, int64_t n, const r3d_poisson_params *params,
                            int64_t cap_vertices, int64_t cap_triangles, double *vertices, double *densities, double *vertex_colors, int32_t *triangles,
                            int64_t *out_nv, int64_t *out_nt) {
    R3D_ROCTX_RANGE("r3d_poisson_reconstruct");
    if (!ctx) return R3D_E_BADARG;
    const char *who = "poisson_reconstruct";
    r3d_poisson_params p;
    int rc;
    if ((rc = po_in_args_ok(ctx, who, xyz, normals, n, params, p)) ||
        (rc = po_out_args_ok(ctx, who, colors != nullptr, cap_vertices, cap_triangles, vertices, densities, vertex_colors, triangles, out_nv, out_nt)))
        return rc;
    *out_nv = *out_nt = 0;
    R3D_HIP(ctx, hipSetDevice(ctx->device));
    DevArena ar(ctx);
    const double *d_xyz, *d_nrm, *d_col;
    if ((rc = r3d_upload(ctx, ar, xyz, (size_t)n * 3, &d_xyz)) || (rc = r3d_upload(ctx, ar, normals, (size_t)n * 3, &d_nrm)) ||
        (rc = r3d_upload(ctx, ar, colors, (size_t)n * 3, &d_col)))
        return rc;
    PoFields F;
    if ((rc = po_solve(ctx, ar, d_xyz, d_nrm, d_col, n, p, p.cycles, F))) return rc;
    PoMeshWork W;
    W.g = F.g; W.chi = F.chi; W.W0 = F.W0; W.C0 = F.C0;
    return po_mesh_to_host(ctx, ar, who, W, cap_vertices, cap_triangles, vertices, densities, vertex_colors, triangles, out_nv, out_nt);
}

int r3d_poisson_reconstruct_dev(r3d_ctx *ctx, const double *d_xyz, const double *d_normals, const double *d_colors, int64_t n,
                                const r3d_poisson_params *params, int64_t cap_vertices, int64_t cap_triangles, double *d_vertices, double *d_densities,
                                double *d_vertex_colors, int32_t *d_triangles, int64_t *out_nv, int64_t *out_nt) {
    R3D_ROCTX_RANGE("r3d_poisson_reconstruct_dev");
    if (!ctx) return R3D_E_BADARG;
    const char *who = "poisson_reconstruct_dev";
    r3d_poisson_params p;
    int rc;
    if ((rc = po_in_args_ok(ctx, who, d_xyz, d_normals, n, params, p)) ||
        (rc = po_out_args_ok(ctx, who, d_colors != nullptr, cap_vertices, cap_triangles, d_vertices, d_densities, d_vertex_colors, d_triangles, out_nv, out_nt)))
        return rc;
    *out_nv = *out_nt = 0;
    R3D_HIP(ctx, hipSetDevice(ctx->device));
    DevArena ar(ctx);
    PoFields F;
    if ((rc = po_solve(ctx, ar, d_xyz, d_normals, d_colors, n, p, p.cycles, F))) return rc;
    PoMeshWork W;
    W.g = F.g; W.chi = F.chi; W.W0 = F.W0; W.C0 = F.C0;
    if ((rc = po_mesh_count(ctx, ar, W, out_nv, out_nt))) return rc;
    if ((cap_vertices > 0 || cap_triangles > 0) && (W.total[0] > 0 || W.total[1] > 0) &&
        ((rc = po_fits(ctx, who, W, cap_vertices, cap_triangles)) || (rc = po_mesh_emit(ctx, W, d_vertices, d_densities, d_vertex_colors, d_triangles))))
        return rc;
    r3d_prof_end(ctx, ctx->ws[0], ctx->stream);
    R3D_HIP(ctx, hipStreamSynchronize(ctx->stream));   // the emitting kernels read arena buffers the next call may hand out again
    return R3D_OK;
}

int r3d_debug_poisson_fields(r3d_ctx *ctx, const double *xyz, const double *normals, const double *colors, int64_t n, const r3d_poisson_params *params,
                             int32_t k_cycles, double *grid4, double *W0, double *C0, double *dens, double *V, double *D, double *b, double *chi) {
    R3D_ROCTX_RANGE("r3d_debug_poisson_fields");
    if (!ctx) return R3D_E_BADARG;
    r3d_poisson_params p;
    int rc;
    if ((rc = po_in_args_ok(ctx, "debug_poisson_fields", xyz, normals, n, params, p))) return rc;
    if (k_cycles < 0 || k_cycles > p.cycles || (C0 && !colors))
        return r3d_fail(ctx, R3D_E_BADARG, "debug_poisson_fields: k_cycles outside 0..cycles, or C0 without colours");
    R3D_HIP(ctx, hipSetDevice(ctx->device));
    DevArena ar(ctx);
    const double *d_xyz, *d_nrm, *d_col;
    if ((rc = r3d_upload(ctx, ar, xyz, (size_t)n * 3, &d_xyz)) || (rc = r3d_upload(ctx, ar, normals, (size_t)n * 3, &d_nrm)) ||
        (rc = r3d_upload(ctx, ar, colors, (size_t)n * 3, &d_col)))
        return rc;
    PoFields F;
    if ((rc = po_solve(ctx, ar, d_xyz, d_nrm, d_col, n, p, k_cycles, F))) return rc;
    if (grid4) { for (int a = 0; a < 3; a++) grid4[a] = F.g.org[a]; grid4[3] = F.g.h; }
    if ((rc = r3d_download(ctx, W0, (const double *)F.W0, F.G3)) || (rc = r3d_download(ctx, C0, (const double *)F.C0, F.C0 ? F.G3 * 3 : 0)) ||
        (rc = r3d_download(ctx, dens, (const double *)F.dens, (size_t)n)) || (rc = r3d_download(ctx, V, (const double *)F.V, F.G3 * 3)) ||
        (rc = r3d_download(ctx, D, (const double *)F.D, F.G3)) || (rc = r3d_download(ctx, b, (const double *)F.b, F.G3)) ||
        (rc = r3d_download(ctx, chi, (const double *)F.chi, F.G3)))
        return rc;
    r3d_prof_end(ctx, ctx->ws[0], ctx->stream);
    R3D_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return R3D_OK;
}

int r3d_debug_poisson_extract(r3d_ctx *ctx, int32_t depth, const double *org3, double h, const double *chi, const double *W0, const double *C0,
                              int64_t cap_vertices, int64_t cap_triangles, double *vertices, double *densities, double *vertex_colors, int32_t *triangles,
                              int64_t *out_nv, int64_t *out_nt) {
    R3D_ROCTX_RANGE("r3d_debug_poisson_extract");
    if (!ctx) return R3D_E_BADARG;
    const char *who = "debug_poisson_extract";
    if (!org3 || !chi || !W0 || !(h > 0.0) || !std::isfinite(h)) return r3d_fail(ctx, R3D_E_BADARG, "%s: a missing array or a cell size that is not positive", who);
    if (depth < 1 || depth > 8) return r3d_fail(ctx, R3D_E_UNSUPPORTED, "%s: depth %d is outside 1..8", who, depth);
    int rc;
    if ((rc = po_out_args_ok(ctx, who, C0 != nullptr, cap_vertices, cap_triangles, vertices, densities, vertex_colors, triangles, out_nv, out_nt))) return rc;
    *out_nv = *out_nt = 0;
    R3D_HIP(ctx, hipSetDevice(ctx->device));
    DevArena ar(ctx);
    PoMeshWork W;
    W.g.R = 1 << depth;
    W.g.G = W.g.R + 1;
    W.g.h = h;
    for (int a = 0; a < 3; a++) W.g.org[a] = org3[a];
    const size_t G3 = (size_t)W.g.G * W.g.G * W.g.G;
    if ((rc = r3d_upload(ctx, ar, chi, G3, &W.chi)) || (rc = r3d_upload(ctx, ar, W0, G3, &W.W0)) || (rc = r3d_upload(ctx, ar, C0, G3 * 3, &W.C0))) return rc;
    r3d_prof_begin(ctx, ctx->ws[0]);
    r3d_prof_mark(ctx, ctx->ws[0], ctx->stream, "poisson_extraction");
    return po_mesh_to_host(ctx, ar, who, W, cap_vertices, cap_triangles, vertices, densities, vertex_colors, triangles, out_nv, out_nt);
}

}  // extern "C"
