// Pose-graph optimisation ("Pose-graph optimisation"): Open3D's global_optimization with the Levenberg-Marquardt
// method on the device.  float64 throughout, every sum in a fixed order, products and additions rounded separately (build.sh passes
// -ffp-contract=off; no f64 MFMA, which fuses), so the result is bit for bit the restatement's (tests/posegraph_ref.py).
//
// A trial builds A = tril(H) + lambda I, factors it by a right-looking tiled Cholesky (per panel of PG_NB columns: the diagonal tile,
// the rows below it, the trailing lower triangle tile by tile through LDS), substitutes forward and back in blocks of PG_SB, and then
// decides.  Every entry of L sees its products in ascending k whatever the tile, which is what makes the tile invisible.  The LM
// decisions live in a PgState block on the device; a kernel enqueued after a stop returns at once; the host reads the first 64 bytes
// of that block once per trial.
#include <algorithm>
#include <cstring>

#include "r3d_internal.h"

namespace {

constexpr int PG_MAX_NODES = 1024;
constexpr int PG_MAX_EDGES = 1 << 20;
constexpr int PG_NB = 32;    // panel width of the factorisation
constexpr int PG_TT = 64;    // side of a trailing-update tile (256 threads, 4 x 4 entries each)
constexpr int PG_SB = 64;    // block of the substitutions

enum { PG_STOP_NONE = 0, PG_STOP_RIGHT_TERM, PG_STOP_INCREMENT, PG_STOP_RESIDUAL_INCREMENT, PG_STOP_RESIDUAL, PG_STOP_ITERATIONS, PG_STOP_NO_EDGES };
enum { PG_ERR_NODE = 1, PG_ERR_SELF = 2, PG_ERR_FINITE = 3 };

struct PgState {
    // the 64 bytes the host reads once per trial
    int32_t stop, error, outer, trials, rejected, failed, inner, pruned;
    double lambda, nu, F, F_first;
    // device only
    double mu, F_new, F_old, den;
    int32_t fail_col, skip, live, relin, accepted, trace_row, pad0, pad1;
};
static_assert(offsetof(PgState, mu) == 64, "the published head of PgState is 64 bytes");

struct PgCrit {
    double min_increment, min_residual_increment, min_right_term, min_residual, prune_threshold, preference, max_distance;
    int ref, max_iteration, max_iteration_lm, trace_cap;
};

// ---- the contract's own sine and cosine (tests/posegraph_ref.py: sincos) ----------------------------------------------------------
__device__ inline void pg_sincos(double x, double &sn, double &cs) {
    if (!(fabs(x) < 1073741824.0)) { sn = cs = NAN; return; }
    const double k = rint(x * 6.36619772367581382433e-01);
    const double r = ((x - k * 1.57079632673412561417e+00) - k * 6.07710050650619224932e-11) - k * 2.02226624879595063154e-21;
    const double z = r * r;
    const double S[9] = {-1.0 / 6.0, 1.0 / 120.0, -1.0 / 5040.0, 1.0 / 362880.0, -1.0 / 39916800.0, 1.0 / 6227020800.0, -1.0 / 1307674368000.0,
                         1.0 / 355687428096000.0, -1.0 / 121645100408832000.0};
    const double C[9] = {-1.0 / 2.0, 1.0 / 24.0, -1.0 / 720.0, 1.0 / 40320.0, -1.0 / 3628800.0, 1.0 / 479001600.0, -1.0 / 87178291200.0,
                         1.0 / 20922789888000.0, -1.0 / 6402373705728000.0};
    double ps = S[8], pc = C[8];
#pragma unroll
    for (int i = 7; i >= 0; i--) { ps = ps * z + S[i]; pc = pc * z + C[i]; }
    const double s = r + r * (z * ps), c = 1.0 + z * pc;
    switch ((int)((long long)k & 3)) {
        case 0: sn = s; cs = c; break;
        case 1: sn = c; cs = -s; break;
        case 2: sn = -s; cs = -c; break;
        default: sn = -c; cs = s; break;
    }
}

// ---- 4x4 algebra, row-major ------------------------------------------------------------------------------------------------------
__device__ inline void pg_mul4(const double *A, const double *B, double *C) {
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) C[i * 4 + j] = ((A[i * 4] * B[j] + A[i * 4 + 1] * B[4 + j]) + A[i * 4 + 2] * B[8 + j]) + A[i * 4 + 3] * B[12 + j];
}
__device__ inline void pg_inv_rigid(const double *X, double *O) {
#pragma unroll
    for (int a = 0; a < 3; a++) {
#pragma unroll
        for (int c = 0; c < 3; c++) O[a * 4 + c] = X[c * 4 + a];
        O[a * 4 + 3] = -((X[a] * X[3] + X[4 + a] * X[7]) + X[8 + a] * X[11]);
    }
    O[12] = O[13] = O[14] = 0.0;
    O[15] = 1.0;
}
__device__ inline void pg_vec6(const double *M, double *v) {
    v[0] = (M[9] - M[6]) * 0.5; v[1] = (M[2] - M[8]) * 0.5; v[2] = (M[4] - M[1]) * 0.5;
    v[3] = M[3]; v[4] = M[7]; v[5] = M[11];
}
__device__ inline void pg_exp6(const double *d, double *U) {
    double sa, ca, sb, cb, sc, cc;
    pg_sincos(d[0], sa, ca);
    pg_sincos(d[1], sb, cb);
    pg_sincos(d[2], sc, cc);
    U[0] = cc * cb; U[1] = cc * sb * sa - sc * ca; U[2] = cc * sb * ca + sc * sa; U[3] = d[3];
    U[4] = sc * cb; U[5] = sc * sb * sa + cc * ca; U[6] = sc * sb * ca - cc * sa; U[7] = d[4];
    U[8] = -sb; U[9] = cb * sa; U[10] = cb * ca; U[11] = d[5];
    U[12] = U[13] = U[14] = 0.0; U[15] = 1.0;
}

// ---- validation: nothing below uses a node id as an address before the host has seen error == 0 --------------------------------------
__global__ void __launch_bounds__(256) k_pg_validate(int N, int E, const double *__restrict__ poses, const int *__restrict__ nodes,
                                                     const double *__restrict__ T, const double *__restrict__ info, const double *__restrict__ conf,
                                                     PgState *st) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    int err = 0;
    if (i < N)
        for (int q = 0; q < 16; q++) if (!isfinite(poses[(size_t)i * 16 + q])) err = PG_ERR_FINITE;
    if (i < E) {
        const int s = nodes[2 * i], t = nodes[2 * i + 1];
        for (int q = 0; q < 16; q++) if (!isfinite(T[(size_t)i * 16 + q])) err = PG_ERR_FINITE;
        for (int q = 0; q < 36; q++) if (!isfinite(info[(size_t)i * 36 + q])) err = PG_ERR_FINITE;
        if (!isfinite(conf[i])) err = PG_ERR_FINITE;
        if (s == t) err = PG_ERR_SELF;
        if (s < 0 || s >= N || t < 0 || t >= N) err = PG_ERR_NODE;
    }
    if (err) atomicMax(&st->error, err);
}

// gates of the kernels that run once per trial whatever the trial decided
enum { PG_GATE_NONE = 0, PG_GATE_TRIAL = 1, PG_GATE_RELIN = 2 };
__device__ inline bool pg_gate_closed(const PgState *st, int gate) {
    if (gate == PG_GATE_TRIAL) return !st->live || st->skip;
    if (gate == PG_GATE_RELIN) return !st->relin;
    return false;
}

// ---- per edge: e, q = e' L e, and (full) W = J' (L J), gr = J' (L e) ---------------------------------------------------------------
__global__ void __launch_bounds__(64) k_pg_edges(int E, const double *__restrict__ X, const int *__restrict__ nodes, const double *__restrict__ T,
                                                 const double *__restrict__ info, int full, double *__restrict__ e_out, double *__restrict__ q_out,
                                                 double *__restrict__ W_out, double *__restrict__ gr_out, const PgState *st, int gate) {
    if (pg_gate_closed(st, gate)) return;
    const int k = blockIdx.x * 64 + threadIdx.x;
    if (k >= E) return;
    const int s = nodes[2 * k], t = nodes[2 * k + 1];
    double Tk[16], Xt[16], Xs[16], A[16], B[16], P[16], e[6], Le[6], L[36];
    for (int q = 0; q < 16; q++) { Tk[q] = T[(size_t)k * 16 + q]; Xt[q] = X[(size_t)t * 16 + q]; Xs[q] = X[(size_t)s * 16 + q]; }
    for (int q = 0; q < 36; q++) L[q] = info[(size_t)k * 36 + q];
    pg_inv_rigid(Tk, A);
    pg_inv_rigid(Xt, B);
    pg_mul4(A, B, P);
    pg_mul4(P, Xs, A);
    pg_vec6(A, e);
    for (int p = 0; p < 6; p++) {
        double acc = L[p * 6] * e[0];
        for (int q = 1; q < 6; q++) acc = acc + L[p * 6 + q] * e[q];
        Le[p] = acc;
    }
    double qq = e[0] * Le[0];
    for (int p = 1; p < 6; p++) qq = qq + e[p] * Le[p];
    q_out[k] = qq;
    if (e_out) for (int p = 0; p < 6; p++) e_out[(size_t)k * 6 + p] = e[p];
    if (!full) return;
    double J[36], LJ[36];   // J[p * 6 + c]: component p of column c
    for (int c = 0; c < 6; c++) {
        double G[16], col[6];
        for (int q = 0; q < 16; q++) G[q] = 0.0;
        if (c == 0) { G[6] = -1.0; G[9] = 1.0; }
        else if (c == 1) { G[2] = 1.0; G[8] = -1.0; }
        else if (c == 2) { G[1] = -1.0; G[4] = 1.0; }
        else G[(c - 3) * 4 + 3] = 1.0;
        pg_mul4(G, Xs, A);
        pg_mul4(P, A, B);
        pg_vec6(B, col);
        for (int p = 0; p < 6; p++) J[p * 6 + c] = col[p];
    }
    for (int p = 0; p < 6; p++)
        for (int c = 0; c < 6; c++) {
            double acc = L[p * 6] * J[c];
            for (int q = 1; q < 6; q++) acc = acc + L[p * 6 + q] * J[q * 6 + c];
            LJ[p * 6 + c] = acc;
        }
    for (int a = 0; a < 6; a++) {
        for (int c = 0; c < 6; c++) {
            double acc = J[a] * LJ[c];
            for (int p = 1; p < 6; p++) acc = acc + J[p * 6 + a] * LJ[p * 6 + c];
            W_out[(size_t)k * 36 + a * 6 + c] = acc;
        }
        double acc = J[a] * Le[0];
        for (int p = 1; p < 6; p++) acc = acc + J[p * 6 + a] * Le[p];
        gr_out[(size_t)k * 6 + a] = acc;
    }
}

// ---- H and b: one wave per node owns the six rows of that node, walks the edges in ascending index and adds those that touch it ----
__global__ void __launch_bounds__(64) k_pg_rows(int E, const int *__restrict__ nodes, const uint8_t *__restrict__ kept, const uint8_t *__restrict__ unc,
                                                const double *__restrict__ conf, const double *__restrict__ W, const double *__restrict__ gr,
                                                double *H, double *__restrict__ b, int n, const PgState *st, int gate) {
    if (pg_gate_closed(st, gate)) return;
    const int i = blockIdx.x, lane = threadIdx.x;
    const int width = 6 * i + 6;
    for (int idx = lane; idx < 6 * width; idx += 64) H[(size_t)(6 * i + idx / width) * n + idx % width] = 0.0;
    __syncthreads();
    const int a = lane < 36 ? lane / 6 : lane - 36, c = lane % 6;
    double acc = 0.0;   // lanes 0..35: entry (a, c) of the diagonal block; lanes 36..41: entry a of b
    for (int base = 0; base < E; base += 64) {
        const int k = base + lane;
        int s = -1, t = -1;
        if (k < E && kept[k]) { s = nodes[2 * k]; t = nodes[2 * k + 1]; }
        unsigned long long m = __ballot(s == i || t == i);
        while (m) {
            const int bit = __ffsll((long long)m) - 1;
            m &= m - 1;
            const int kk = base + bit, ss = __shfl(s, bit), tt = __shfl(t, bit);
            const double l = unc[kk] ? conf[kk] : 1.0;
            if (lane < 36) {
                const double w = l * W[(size_t)kk * 36 + a * 6 + c];
                acc = acc + w;
                const int other = ss == i ? tt : ss;
                if (other < i) {
                    if (ss == i) H[(size_t)(6 * i + a) * n + 6 * other + c] -= w;   // s > t: block (s, t) -= Wl
                    else H[(size_t)(6 * i + c) * n + 6 * other + a] -= w;           // s < t: block (t, s) -= Wl'
                }
            } else if (lane < 42) {
                const double g = l * gr[(size_t)kk * 6 + a];
                acc = ss == i ? acc + g : acc - g;
            }
        }
    }
    if (lane < 36) { if (c <= a) H[(size_t)(6 * i + a) * n + 6 * i + c] = acc; }
    else if (lane < 42) b[6 * i + a] = acc;
}

// dense symmetric copy of the lower triangle (the debug entry's H)
__global__ void __launch_bounds__(256) k_pg_mirror(const double *__restrict__ H, double *__restrict__ out, int n) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)n * n) return;
    const int i = (int)(idx / n), j = (int)(idx % n);
    out[idx] = i >= j ? H[idx] : H[(size_t)j * n + i];
}
// the debug entry's L: the lower triangle, zero above it; all zero after a failed pivot
__global__ void __launch_bounds__(256) k_pg_lower(const double *__restrict__ A, double *__restrict__ out, int n, const PgState *st) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)n * n) return;
    const int i = (int)(idx / n), j = (int)(idx % n);
    out[idx] = (i >= j && st->fail_col < 0) ? A[idx] : 0.0;
}
__global__ void __launch_bounds__(256) k_pg_delta_out(const double *__restrict__ x, double *__restrict__ out, int n, const PgState *st) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = st->fail_col < 0 ? x[i] : 0.0;
}

// F = (sum of l q over the kept edges) + (sum of mu (sqrt l - 1)^2 over the uncertain kept edges), both in ascending edge index
__device__ double pg_objective(int E, const double *q, const uint8_t *kept, const uint8_t *unc, const double *conf, double mu) {
    double F1 = 0.0, F2 = 0.0;
    for (int k = 0; k < E; k++) {
        if (!kept[k]) continue;
        const double l = unc[k] ? conf[k] : 1.0;
        F1 = F1 + l * q[k];
        if (unc[k]) { const double d = sqrt(l) - 1.0; F2 = F2 + mu * (d * d); }
    }
    return F1 + F2;
}
__device__ double pg_block_max(double v, double *sh) {   // the maximum over the 256 threads of a block (order does not matter to a maximum)
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) sh[threadIdx.x] = fmax(sh[threadIdx.x], sh[threadIdx.x + w]);
        __syncthreads();
    }
    const double r = sh[0];
    __syncthreads();
    return r;
}
__device__ inline void pg_trace(PgState *st, double *trace, int cap, double lam, double Fn, double rho, double code) {
    if (trace && st->trace_row < cap) {
        double *r = trace + (size_t)st->trace_row * 4;
        r[0] = lam; r[1] = Fn; r[2] = rho; r[3] = code;
    }
    st->trace_row++;
}

// start of an optimisation, after the first linearisation: mu, F, lambda0 and the right-term test
__global__ void __launch_bounds__(256) k_pg_begin(int E, int n, const double *__restrict__ H, const double *__restrict__ b, const double *__restrict__ q,
                                                  const uint8_t *__restrict__ kept, const uint8_t *__restrict__ unc, const double *__restrict__ conf,
                                                  const double *__restrict__ info, PgCrit cr, PgState *st) {
    __shared__ double sh[256];
    double md = -INFINITY, mb = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) { md = fmax(md, H[(size_t)i * n + i]); mb = fmax(mb, fabs(b[i])); }
    md = pg_block_max(md, sh);
    mb = pg_block_max(mb, sh);
    if (threadIdx.x) return;
    int cnt = 0;
    double sum = 0.0;
    for (int k = 0; k < E; k++)
        if (kept[k]) { sum = cnt ? sum + info[(size_t)k * 36 + 35] : info[(size_t)k * 36 + 35]; cnt++; }
    st->stop = PG_STOP_NONE; st->outer = 0; st->inner = 0; st->live = 0; st->skip = 0; st->relin = 0; st->accepted = 0; st->fail_col = -1;
    if (!cnt) { st->stop = PG_STOP_NO_EDGES; st->mu = 0.0; st->F = st->F_first = 0.0; return; }
    const double mean = sum / (double)cnt;
    st->mu = ((cr.preference * cr.max_distance) * cr.max_distance) * mean;
    st->F = st->F_first = pg_objective(E, q, kept, unc, conf, st->mu);
    st->lambda = 1e-5 * md;
    st->nu = 2.0;
    if (mb < cr.min_right_term) st->stop = PG_STOP_RIGHT_TERM;
    else if (cr.max_iteration == 0 || cr.max_iteration_lm == 0) st->stop = PG_STOP_ITERATIONS;
}

// ---- a trial: A = tril(H) + lambda I, c = -b ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_pg_form(const double *__restrict__ H, const double *__restrict__ b, double *__restrict__ A, double *__restrict__ c,
                                                 int n, double lam_arg, int use_state, PgState *st) {
    if (st->stop) return;
    if (blockIdx.y * 16 > blockIdx.x * 16 + 15) return;   // a tile above the diagonal
    const int i = blockIdx.x * 16 + threadIdx.y, j = blockIdx.y * 16 + threadIdx.x;
    const double lam = use_state ? st->lambda : lam_arg;
    if (i < n && j <= i) A[(size_t)i * n + j] = i == j ? H[(size_t)i * n + j] + lam : H[(size_t)i * n + j];
    if (blockIdx.y == 0 && threadIdx.x == 0 && i < n) c[i] = -b[i];
}
__device__ inline bool pg_solve_off(const PgState *st) { return st->stop || st->fail_col >= 0; }

// One panel: every workgroup factors the 32 x 32 diagonal tile for itself in LDS (a thread per entry, right-looking, three barriers
// per pivot), then each thread takes one row below the tile: L[i][j] = (A[i][j] - sum_{k<j in the panel} L[i][k] L[j][k]) / L[j][j].
// The tile in A is read by every workgroup, so workgroup 0 publishes the factored tile to `tile_out` and k_pg_trail copies it into
// A; a panel with no rows below is a single workgroup and writes A itself.  A pivot <= 0 or not finite is recorded and ends the
// factorisation: every workgroup sees it and returns before it writes anything.
__global__ void __launch_bounds__(1024) k_pg_panel(double *A, int n, int p0, double *__restrict__ tile_out, PgState *st) {
    if (pg_solve_off(st)) return;
    __shared__ double D[PG_NB][PG_NB + 1];
    __shared__ int fail;
    const int nb = min(PG_NB, n - p0), r = threadIdx.x / PG_NB, c = threadIdx.x % PG_NB;
    D[r][c] = (r < nb && c <= r) ? A[(size_t)(p0 + r) * n + p0 + c] : 0.0;
    if (threadIdx.x == 0) fail = -1;
    __syncthreads();
    for (int j = 0; j < nb; j++) {
        const double v = D[j][j];
        if (!(v > 0.0 && isfinite(v))) { if (threadIdx.x == 0) fail = j; break; }   // every thread sees the same v
        const double d = sqrt(v);
        __syncthreads();
        if (c == j && r == j) D[j][j] = d;
        if (c == j && r > j && r < nb) D[r][j] = D[r][j] / d;
        __syncthreads();
        if (c > j && r >= c && r < nb) D[r][c] = D[r][c] - D[r][j] * D[c][j];
        __syncthreads();
    }
    __syncthreads();
    if (fail >= 0) { if (blockIdx.x == 0 && threadIdx.x == 0) st->fail_col = p0 + fail; return; }
    if (blockIdx.x == 0 && r < nb && c <= r) {
        if (gridDim.x == 1 && n - p0 <= PG_NB) A[(size_t)(p0 + r) * n + p0 + c] = D[r][c];
        else tile_out[r * PG_NB + c] = D[r][c];
    }
    const int i = p0 + PG_NB + blockIdx.x * 1024 + threadIdx.x;
    if (i >= n) return;
    double row[PG_NB];
    double *src = A + (size_t)i * n + p0;
#pragma unroll
    for (int j = 0; j < PG_NB; j++) row[j] = src[j];
#pragma unroll
    for (int j = 0; j < PG_NB; j++) {
        double v = row[j];
#pragma unroll
        for (int k = 0; k < j; k++) v = v - row[k] * D[j][k];
        row[j] = v / D[j][j];
    }
#pragma unroll
    for (int j = 0; j < PG_NB; j++) src[j] = row[j];
}
// the trailing update of one 64 x 64 tile at or below the diagonal: A[i][j] -= L[i][k] L[j][k] for the panel's k in ascending order
__global__ void __launch_bounds__(256) k_pg_trail(double *A, int n, int p0, const double *__restrict__ tile_in, const PgState *st) {
    if (pg_solve_off(st)) return;
    if (blockIdx.y > blockIdx.x) return;
    if (blockIdx.x == 0)   // the panel's factored diagonal tile goes home; nothing reads that part of A here
        for (int idx = threadIdx.x; idx < PG_NB * PG_NB; idx += 256)
            if (idx % PG_NB <= idx / PG_NB) A[(size_t)(p0 + idx / PG_NB) * n + p0 + idx % PG_NB] = tile_in[idx];
    __shared__ double As[PG_NB][PG_TT], Bs[PG_NB][PG_TT];
    const int p1 = p0 + PG_NB, i0 = p1 + blockIdx.x * PG_TT, j0 = p1 + blockIdx.y * PG_TT;
    for (int idx = threadIdx.x; idx < PG_TT * PG_NB; idx += 256) {
        const int r = idx / PG_NB, k = idx % PG_NB;
        As[k][r] = i0 + r < n ? A[(size_t)(i0 + r) * n + p0 + k] : 0.0;
        Bs[k][r] = j0 + r < n ? A[(size_t)(j0 + r) * n + p0 + k] : 0.0;
    }
    __syncthreads();
    const int ty = threadIdx.x / 16, tx = threadIdx.x % 16;
    double acc[4][4];
#pragma unroll
    for (int u = 0; u < 4; u++)
#pragma unroll
        for (int v = 0; v < 4; v++) {
            const int i = i0 + ty * 4 + u, j = j0 + tx * 4 + v;
            acc[u][v] = (i < n && j <= i) ? A[(size_t)i * n + j] : 0.0;
        }
#pragma unroll 4
    for (int k = 0; k < PG_NB; k++) {
        double a[4], b[4];
#pragma unroll
        for (int u = 0; u < 4; u++) { a[u] = As[k][ty * 4 + u]; b[u] = Bs[k][tx * 4 + u]; }
#pragma unroll
        for (int u = 0; u < 4; u++)
#pragma unroll
            for (int v = 0; v < 4; v++) acc[u][v] = acc[u][v] - a[u] * b[v];
    }
#pragma unroll
    for (int u = 0; u < 4; u++)
#pragma unroll
        for (int v = 0; v < 4; v++) {
            const int i = i0 + ty * 4 + u, j = j0 + tx * 4 + v;
            if (i < n && j <= i) A[(size_t)i * n + j] = acc[u][v];
        }
}

// forward substitution, block p0: every workgroup solves the diagonal block for itself (64 steps), block 0 publishes it to y, and
// each thread takes the block out of one later row of c, k ascending.  c's rows of the block are read by all and written by none.
__global__ void __launch_bounds__(256) k_pg_forward(const double *__restrict__ L, double *c, double *__restrict__ y, int n, int p0, const PgState *st) {
    if (pg_solve_off(st)) return;
    __shared__ double D[PG_SB][PG_SB + 1];
    __shared__ double ys[PG_SB];
    const int nb = min(PG_SB, n - p0), r = threadIdx.x;
    for (int idx = r; idx < nb * nb; idx += 256) {
        const int i = idx / nb, j = idx % nb;
        D[i][j] = j <= i ? L[(size_t)(p0 + i) * n + p0 + j] : 0.0;
    }
    if (r < nb) ys[r] = c[p0 + r];
    __syncthreads();
    for (int j = 0; j < nb; j++) {
        if (r == j) ys[j] = ys[j] / D[j][j];
        __syncthreads();
        if (r > j && r < nb) ys[r] = ys[r] - D[r][j] * ys[j];
        __syncthreads();
    }
    if (blockIdx.x == 0 && r < nb) y[p0 + r] = ys[r];
    const int i = p0 + nb + blockIdx.x * 256 + r;
    if (i >= n) return;
    double v = c[i];
    const double *row = L + (size_t)i * n + p0;
    for (int k = 0; k < nb; k++) v = v - row[k] * ys[k];
    c[i] = v;
}
// back substitution, block p0 (blocks in descending order): x[i] = (y[i] - sum_{k>i} L[k][i] x[k]) / L[i][i], k descending
__global__ void __launch_bounds__(256) k_pg_backward(const double *__restrict__ L, double *y, double *__restrict__ x, int n, int p0, const PgState *st) {
    if (pg_solve_off(st)) return;
    __shared__ double D[PG_SB][PG_SB + 1];
    __shared__ double xs[PG_SB];
    const int nb = min(PG_SB, n - p0), r = threadIdx.x;
    for (int idx = r; idx < nb * nb; idx += 256) {
        const int i = idx / nb, j = idx % nb;
        D[i][j] = j <= i ? L[(size_t)(p0 + i) * n + p0 + j] : 0.0;
    }
    if (r < nb) xs[r] = y[p0 + r];
    __syncthreads();
    for (int j = nb - 1; j >= 0; j--) {
        if (r == j) xs[j] = xs[j] / D[j][j];
        __syncthreads();
        if (r < j) xs[r] = xs[r] - D[j][r] * xs[j];
        __syncthreads();
    }
    if (blockIdx.x == 0 && r < nb) x[p0 + r] = xs[r];
    const int i = blockIdx.x * 256 + r;
    if (i >= p0) return;
    double v = y[i];
    for (int k = nb - 1; k >= 0; k--) v = v - L[(size_t)(p0 + k) * n + i] * xs[k];
    y[i] = v;
}

// after the solve: the step's tests and the trial poses
__global__ void __launch_bounds__(256) k_pg_step(int N, const double *__restrict__ X, double *__restrict__ Xtrial, double *delta, const double *__restrict__ b,
                                                 PgCrit cr, double *trace, PgState *st) {
    __shared__ int go;
    if (threadIdx.x == 0) {
        go = 0;
        if (!st->stop) {
            st->live = 1; st->skip = 0; st->accepted = 0; st->relin = 0;
            st->trials++;
            st->inner++;
            const double lam = st->lambda;
            if (st->fail_col >= 0) {
                st->failed++;
                st->rejected++;
                pg_trace(st, trace, cr.trace_cap, lam, 0.0, 0.0, -2.0);
                st->lambda = lam * st->nu;
                st->nu = st->nu * 2.0;
                st->skip = 1;
            } else {
                const int n = 6 * N;
                if (cr.ref >= 0) for (int q = 0; q < 6; q++) delta[6 * cr.ref + q] = 0.0;
                double dd = delta[0] * delta[0];
                for (int i = 1; i < n; i++) dd = dd + delta[i] * delta[i];
                double xx = 0.0;
                for (int i = 0; i < N; i++) {
                    double v[6];
                    pg_vec6(X + (size_t)i * 16, v);
                    for (int q = 0; q < 6; q++) xx = (i == 0 && q == 0) ? v[q] * v[q] : xx + v[q] * v[q];
                }
                if (sqrt(dd) < cr.min_increment * (sqrt(xx) + cr.min_increment)) {
                    pg_trace(st, trace, cr.trace_cap, lam, 0.0, 0.0, -1.0);
                    st->stop = PG_STOP_INCREMENT;
                    st->skip = 1;
                    st->live = 0;
                } else {
                    double den = delta[0] * (lam * delta[0] - b[0]);
                    for (int i = 1; i < n; i++) den = den + delta[i] * (lam * delta[i] - b[i]);
                    st->den = den + 1e-3;
                    go = 1;
                }
            }
        }
    }
    __syncthreads();
    if (!go) return;
    for (int i = threadIdx.x; i < N; i += 256) {
        double d[6], U[16], Xi[16], O[16];
        for (int q = 0; q < 6; q++) d[q] = delta[6 * i + q];
        for (int q = 0; q < 16; q++) Xi[q] = X[(size_t)i * 16 + q];
        pg_exp6(d, U);
        pg_mul4(U, Xi, O);
        for (int q = 0; q < 16; q++) Xtrial[(size_t)i * 16 + q] = O[q];
    }
}
// rho and the decision; an accepted step moves the poses and recomputes the confidences of the uncertain edges
__global__ void __launch_bounds__(256) k_pg_decide(int N, int E, double *__restrict__ X, const double *__restrict__ Xtrial, const double *__restrict__ q_new,
                                                   const uint8_t *__restrict__ kept, const uint8_t *__restrict__ unc, double *conf, PgCrit cr, double *trace,
                                                   PgState *st) {
    __shared__ int go;
    if (threadIdx.x == 0) {
        go = 0;
        if (st->live && !st->skip) {
            const double lam = st->lambda, Fn = pg_objective(E, q_new, kept, unc, conf, st->mu);
            const double rho = (st->F - Fn) / st->den;
            if (rho > 0.0) {
                pg_trace(st, trace, cr.trace_cap, lam, Fn, rho, 1.0);
                const double t = 2.0 * rho - 1.0, scale = 1.0 - (t * t) * t;
                st->lambda = lam * (scale > 1.0 / 3.0 ? scale : 1.0 / 3.0);
                st->nu = 2.0;
                st->accepted = 1;
                st->relin = 1;
                st->F_old = st->F;
                st->F_new = Fn;
                go = 1;
            } else {
                st->rejected++;
                pg_trace(st, trace, cr.trace_cap, lam, Fn, rho, 0.0);
                st->lambda = lam * st->nu;
                st->nu = st->nu * 2.0;
            }
        }
    }
    __syncthreads();
    if (!go) return;
    const double mu = st->mu;
    for (int i = threadIdx.x; i < N * 16; i += 256) X[i] = Xtrial[i];
    for (int k = threadIdx.x; k < E; k += 256)
        if (unc[k] && kept[k]) { const double r = mu / (mu + q_new[k]); conf[k] = r * r; }
}
// end of a trial: F and the stops of an accepted step (after its re-linearisation), then the iteration counts
__global__ void __launch_bounds__(256) k_pg_after(int E, int n, const double *__restrict__ b, const double *__restrict__ q, const uint8_t *__restrict__ kept,
                                                  const uint8_t *__restrict__ unc, const double *__restrict__ conf, PgCrit cr, PgState *st) {
    __shared__ double sh[256];
    __shared__ int live, relin;
    if (threadIdx.x == 0) { live = st->live; relin = st->relin; }
    __syncthreads();
    if (!live) return;
    double mb = 0.0;
    if (relin) {
        for (int i = threadIdx.x; i < n; i += 256) mb = fmax(mb, fabs(b[i]));
        mb = pg_block_max(mb, sh);
    }
    if (threadIdx.x) return;
    if (relin) {
        st->F = pg_objective(E, q, kept, unc, conf, st->mu);
        if (st->F_old - st->F_new < cr.min_residual_increment * st->F_old) st->stop = PG_STOP_RESIDUAL_INCREMENT;
        else if (st->F_new < cr.min_residual) st->stop = PG_STOP_RESIDUAL;
        else if (mb < cr.min_right_term) st->stop = PG_STOP_RIGHT_TERM;
        st->relin = 0;
    }
    if (st->accepted || st->inner >= cr.max_iteration_lm) {
        st->outer++;
        st->inner = 0;
        if (st->outer >= cr.max_iteration && st->stop == PG_STOP_NONE) st->stop = PG_STOP_ITERATIONS;
    }
    st->live = 0;
    st->fail_col = -1;
}

__global__ void __launch_bounds__(256) k_pg_keep_all(int E, uint8_t *kept) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k < E) kept[k] = 1;
}
__global__ void __launch_bounds__(256) k_pg_prune(int E, const uint8_t *__restrict__ unc, const double *__restrict__ conf, double thr, uint8_t *__restrict__ kept,
                                                  PgState *st) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= E) return;
    const bool drop = unc[k] && conf[k] < thr;
    kept[k] = drop ? 0 : 1;
    if (drop) atomicAdd(&st->pruned, 1);
}
// the reference node ends where it began: if its pose changed, every pose is multiplied from the left by before * inv_rigid(after)
__global__ void __launch_bounds__(256) k_pg_gauge(int N, double *X, const double *__restrict__ before, int ref) {
    __shared__ double M[16];
    __shared__ int changed;
    if (threadIdx.x == 0) {
        changed = 0;
        for (int q = 0; q < 16; q++) if (!(X[(size_t)ref * 16 + q] == before[q])) changed = 1;
        if (changed) {
            double A[16], B[16], I[16], O[16];
            for (int q = 0; q < 16; q++) { A[q] = before[q]; B[q] = X[(size_t)ref * 16 + q]; }
            pg_inv_rigid(B, I);
            pg_mul4(A, I, O);
            for (int q = 0; q < 16; q++) M[q] = O[q];
        }
    }
    __syncthreads();
    if (!changed) return;
    for (int i = threadIdx.x; i < N; i += 256) {
        double A[16], Xi[16], O[16];
        for (int q = 0; q < 16; q++) { A[q] = M[q]; Xi[q] = X[(size_t)i * 16 + q]; }
        pg_mul4(A, Xi, O);
        for (int q = 0; q < 16; q++) X[(size_t)i * 16 + q] = O[q];
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
const r3d_posegraph_params PG_DEFAULTS = {0.03, 0.25, 1.0, 1e-6, 1e-6, 1e-6, 1e-6, -1, 100, 20, 0};

struct PgWork {
    int N = 0, E = 0, n = 0;
    double *X = nullptr, *conf = nullptr;          // in / out (the caller's arrays in the _dev form)
    uint8_t *kept = nullptr;
    const int *nodes = nullptr;
    const double *T = nullptr, *info = nullptr;
    const uint8_t *unc = nullptr;
    double *Xtrial = nullptr, *e = nullptr, *q = nullptr, *q_new = nullptr, *W = nullptr, *gr = nullptr, *H = nullptr, *b = nullptr, *A = nullptr,
           *c = nullptr, *y = nullptr, *delta = nullptr, *trace = nullptr, *before = nullptr, *tile = nullptr;
    PgState *st = nullptr;
    PgCrit cr = {};
    r3d_events<5> ev;
    double ms[4] = {0, 0, 0, 0};   // linearise, factor, substitute, rest
};

int pg_params_ok(r3d_ctx *ctx, const char *who, const r3d_posegraph_params *params, r3d_posegraph_params &p, int64_t N) {
    p = params ? *params : PG_DEFAULTS;
    if (N < 1 || N > PG_MAX_NODES) return r3d_fail(ctx, R3D_E_BADARG, "%s: %lld nodes (1..%d are supported)", who, (long long)N, PG_MAX_NODES);
    if (p.reference_node < -1 || p.reference_node >= N)
        return r3d_fail(ctx, R3D_E_BADARG, "%s: reference_node %d is outside -1..%lld", who, p.reference_node, (long long)N - 1);
    if (p.max_iteration < 0 || p.max_iteration_lm < 0 || p.trace_capacity < 0)
        return r3d_fail(ctx, R3D_E_BADARG, "%s: a negative iteration count or trace capacity", who);
    const double d[7] = {p.max_correspondence_distance, p.edge_prune_threshold, p.preference_loop_closure, p.min_relative_increment,
                         p.min_relative_residual_increment, p.min_right_term, p.min_residual};
    for (double v : d) if (!std::isfinite(v)) return r3d_fail(ctx, R3D_E_BADARG, "%s: a parameter that is not finite", who);
    return R3D_OK;
}
PgCrit pg_crit(const r3d_posegraph_params &p) {
    PgCrit c;
    c.min_increment = p.min_relative_increment; c.min_residual_increment = p.min_relative_residual_increment;
    c.min_right_term = p.min_right_term; c.min_residual = p.min_residual; c.prune_threshold = p.edge_prune_threshold;
    c.preference = p.preference_loop_closure; c.max_distance = p.max_correspondence_distance;
    c.ref = p.reference_node; c.max_iteration = p.max_iteration; c.max_iteration_lm = p.max_iteration_lm; c.trace_cap = p.trace_capacity;
    return c;
}

// the published 64 bytes of the state block, through the context's pinned buffer
int pg_read_state(r3d_ctx *ctx, const PgState *d_st, PgState &h) {
    if (!ctx->pin.p) {
        hipError_t e = ctx->pin.alloc(R3D_PIN_BYTES, hipHostMallocMapped);
        if (e != hipSuccess) return r3d_fail(ctx, R3D_E_OOM, "hipHostMalloc(%d) failed: %s", R3D_PIN_BYTES, hipGetErrorString(e));
        memset(ctx->pin.p, 0, 64);
    }
    char *land = (char *)ctx->pin.p + 64;
    R3D_HIP(ctx, hipMemcpyAsync(land, d_st, 64, hipMemcpyDeviceToHost, ctx->stream));
    R3D_HIP(ctx, hipStreamSynchronize(ctx->stream));
    memcpy(&h, land, 64);
    return R3D_OK;
}

int pg_alloc(r3d_ctx *ctx, DevArena &ar, PgWork &W, bool solver) {
    const size_t N = W.N, E = W.E, n = W.n;
    if (E == 0) {   // nothing to optimise: the state block alone, for the validation of the poses
        W.st = (PgState *)ar.get(sizeof(PgState));
        if (ar.rc) return ar.rc;
        R3D_HIP(ctx, hipMemsetAsync(W.st, 0, sizeof(PgState), ctx->stream));
        return R3D_OK;
    }
    W.Xtrial = (double *)ar.get(N * 16 * 8);
    W.e = (double *)ar.get(E * 6 * 8);
    W.q = (double *)ar.get(E * 8);
    W.q_new = (double *)ar.get(E * 8);
    W.W = (double *)ar.get(E * 36 * 8);
    W.gr = (double *)ar.get(E * 6 * 8);
    W.H = (double *)ar.get(n * n * 8);
    W.b = (double *)ar.get(n * 8);
    if (solver) {
        W.A = (double *)ar.get(n * n * 8);
        W.c = (double *)ar.get(n * 8);
        W.y = (double *)ar.get(n * 8);
        W.delta = (double *)ar.get(n * 8);
        W.tile = (double *)ar.get(PG_NB * PG_NB * 8);
    }
    W.before = (double *)ar.get(16 * 8);
    W.st = (PgState *)ar.get(sizeof(PgState));
    if (ar.rc) return ar.rc;
    R3D_HIP(ctx, hipMemsetAsync(W.st, 0, sizeof(PgState), ctx->stream));
    return R3D_OK;
}

void pg_linearize(r3d_ctx *ctx, PgWork &W, const double *X, int gate) {
    if (W.E) k_pg_edges<<<(W.E + 63) / 64, 64, 0, ctx->stream>>>(W.E, X, W.nodes, W.T, W.info, 1, W.e, W.q, W.W, W.gr, W.st, gate);
    k_pg_rows<<<W.N, 64, 0, ctx->stream>>>(W.E, W.nodes, W.kept, W.unc, W.conf, W.W, W.gr, W.H, W.b, W.n, W.st, gate);
}
// Cholesky of A (lower triangle, in place) and the two substitutions: (L L') delta = c
void pg_factor(r3d_ctx *ctx, double *A, int n, double *tile, PgState *st) {
    hipStream_t s = ctx->stream;
    for (int p0 = 0; p0 < n; p0 += PG_NB) {
        const int below = n - p0 - PG_NB;
        k_pg_panel<<<below > 0 ? (below + 1023) / 1024 : 1, 1024, 0, s>>>(A, n, p0, tile, st);
        if (below <= 0) break;
        const int tiles = (below + PG_TT - 1) / PG_TT;
        k_pg_trail<<<dim3(tiles, tiles), 256, 0, s>>>(A, n, p0, tile, st);
    }
}
void pg_substitute(r3d_ctx *ctx, const double *L, double *c, double *y, double *x, int n, PgState *st) {
    hipStream_t s = ctx->stream;
    for (int p0 = 0; p0 < n; p0 += PG_SB) {
        const int below = n - p0 - PG_SB;
        k_pg_forward<<<below > 0 ? (below + 255) / 256 : 1, 256, 0, s>>>(L, c, y, n, p0, st);
    }
    for (int p0 = (n - 1) / PG_SB * PG_SB; p0 >= 0; p0 -= PG_SB)
        k_pg_backward<<<p0 > 0 ? (p0 + 255) / 256 : 1, 256, 0, s>>>(L, y, x, n, p0, st);
}

// one optimisation of the kept edges; the counts of st accumulate over the passes (trials, rejected, failed, trace_row)
int pg_optimize_pass(r3d_ctx *ctx, PgWork &W, PgState &h) {
    hipStream_t s = ctx->stream;
    const int n = W.n, E = W.E, N = W.N;
    R3D_HIP(ctx, hipEventRecord(W.ev[0], s));
    pg_linearize(ctx, W, W.X, PG_GATE_NONE);
    k_pg_begin<<<1, 256, 0, s>>>(E, n, W.H, W.b, W.q, W.kept, W.unc, W.conf, W.info, W.cr, W.st);
    R3D_HIP(ctx, hipEventRecord(W.ev[1], s));
    R3D_HIP(ctx, hipGetLastError());
    int rc;
    if ((rc = pg_read_state(ctx, W.st, h))) return rc;
    float ms = 0;
    R3D_HIP(ctx, hipEventElapsedTime(&ms, W.ev[0], W.ev[1]));
    W.ms[0] += ms;
    const int64_t bound = (int64_t)W.cr.max_iteration * W.cr.max_iteration_lm;
    const int t16 = (n + 15) / 16;
    for (int64_t trial = 0; !h.stop && trial < bound; trial++) {
        R3D_HIP(ctx, hipEventRecord(W.ev[0], s));
        k_pg_form<<<dim3(t16, t16), dim3(16, 16), 0, s>>>(W.H, W.b, W.A, W.c, n, 0.0, 1, W.st);
        pg_factor(ctx, W.A, n, W.tile, W.st);
        R3D_HIP(ctx, hipEventRecord(W.ev[1], s));
        pg_substitute(ctx, W.A, W.c, W.y, W.delta, n, W.st);
        R3D_HIP(ctx, hipEventRecord(W.ev[2], s));
        k_pg_step<<<1, 256, 0, s>>>(N, W.X, W.Xtrial, W.delta, W.b, W.cr, W.trace, W.st);
        k_pg_edges<<<(E + 63) / 64, 64, 0, s>>>(E, W.Xtrial, W.nodes, W.T, W.info, 0, nullptr, W.q_new, nullptr, nullptr, W.st, PG_GATE_TRIAL);
        k_pg_decide<<<1, 256, 0, s>>>(N, E, W.X, W.Xtrial, W.q_new, W.kept, W.unc, W.conf, W.cr, W.trace, W.st);
        R3D_HIP(ctx, hipEventRecord(W.ev[3], s));
        pg_linearize(ctx, W, W.X, PG_GATE_RELIN);
        k_pg_after<<<1, 256, 0, s>>>(E, n, W.b, W.q, W.kept, W.unc, W.conf, W.cr, W.st);
        R3D_HIP(ctx, hipEventRecord(W.ev[4], s));
        R3D_HIP(ctx, hipGetLastError());
        if ((rc = pg_read_state(ctx, W.st, h))) return rc;
        const int slot[4] = {1, 2, 3, 0};   // factor, substitute, rest, linearise
        for (int k = 0; k < 4; k++) {
            R3D_HIP(ctx, hipEventElapsedTime(&ms, W.ev[k], W.ev[k + 1]));
            W.ms[slot[k]] += ms;
        }
    }
    return R3D_OK;
}

const char *pg_error_text(int e) {
    return e == PG_ERR_NODE ? "an edge names a node outside 0..n_nodes-1" : e == PG_ERR_SELF ? "an edge joins a node to itself"
                                                                                              : "a pose, transformation, information matrix or confidence that is not finite";
}

// validation on the device (both forms take this path), then the host's look at the result
int pg_validate(r3d_ctx *ctx, const char *who, PgWork &W) {
    const int m = std::max(W.N, W.E);
    k_pg_validate<<<(m + 255) / 256, 256, 0, ctx->stream>>>(W.N, W.E, W.X, W.nodes, W.T, W.info, W.conf, W.st);
    R3D_HIP(ctx, hipGetLastError());
    PgState h;
    if (int rc = pg_read_state(ctx, W.st, h)) return rc;
    if (h.error) return r3d_fail(ctx, R3D_E_BADARG, "%s: %s", who, pg_error_text(h.error));
    return R3D_OK;
}

int pg_edge_args_ok(r3d_ctx *ctx, const char *who, int64_t E, const void *nodes, const void *T, const void *info, const void *unc, const void *conf) {
    if (E < 0 || E > PG_MAX_EDGES) return r3d_fail(ctx, R3D_E_BADARG, "%s: %lld edges (0..2^20 are supported)", who, (long long)E);
    if (E > 0 && (!nodes || !T || !info || !unc || !conf)) return r3d_fail(ctx, R3D_E_BADARG, "%s: a missing edge array", who);
    return R3D_OK;
}

// the whole of global_optimization on device arrays; poses and confidences in place
int pg_run(r3d_ctx *ctx, DevArena &ar, const char *who, const r3d_posegraph_params &p, PgWork &W, r3d_posegraph_stats *stats) {
    hipStream_t s = ctx->stream;
    int rc;
    W.n = 6 * W.N;
    W.cr = pg_crit(p);
    if ((rc = pg_alloc(ctx, ar, W, W.E > 0))) return rc;
    r3d_posegraph_stats out = {};
    out.stop_first = out.stop_second = PG_STOP_NO_EDGES;
    if ((rc = pg_validate(ctx, who, W))) return rc;
    if (W.E > 0) {
        if (W.ev.create_all() != hipSuccess) return r3d_fail(ctx, R3D_E_HIP, "%s: hipEventCreate failed", who);
        if (p.reference_node >= 0)
            R3D_HIP(ctx, hipMemcpyAsync(W.before, W.X + (size_t)p.reference_node * 16, 128, hipMemcpyDeviceToDevice, s));
        k_pg_keep_all<<<(W.E + 255) / 256, 256, 0, s>>>(W.E, W.kept);
        PgState h1, h2;
        if ((rc = pg_optimize_pass(ctx, W, h1))) return rc;
        k_pg_prune<<<(W.E + 255) / 256, 256, 0, s>>>(W.E, W.unc, W.conf, p.edge_prune_threshold, W.kept, W.st);
        if ((rc = pg_optimize_pass(ctx, W, h2))) return rc;
        if (p.reference_node >= 0) k_pg_gauge<<<1, 256, 0, s>>>(W.N, W.X, W.before, p.reference_node);
        R3D_HIP(ctx, hipGetLastError());
        out.outer_iterations = h1.outer + h2.outer;
        out.trials = h2.trials;
        out.rejected_trials = h2.rejected;
        out.failed_factorizations = h2.failed;
        out.edges_pruned = h2.pruned;
        out.stop_first = h1.stop;
        out.stop_second = h2.stop;
        out.first_objective = h1.F_first;
        out.final_objective = h2.stop == PG_STOP_NO_EDGES ? h1.F : h2.F;
        out.linearize_ms = W.ms[0]; out.factor_ms = W.ms[1]; out.substitute_ms = W.ms[2]; out.rest_ms = W.ms[3];
    }
    if (stats) *stats = out;
    return R3D_OK;
}

}  // namespace

extern "C" {

int r3d_posegraph_optimize_dev(r3d_ctx *ctx, const r3d_posegraph_params *params, int64_t n_nodes, double *d_poses, int64_t n_edges,
                               const int32_t *d_edge_nodes, const double *d_edge_T, const double *d_edge_info, const uint8_t *d_edge_uncertain,
                               double *d_edge_confidence, uint8_t *d_edge_kept, r3d_posegraph_stats *stats, double *d_trace) {
    R3D_ROCTX_RANGE("r3d_posegraph_optimize_dev");
    if (!ctx) return R3D_E_BADARG;
    const char *who = "posegraph_optimize_dev";
    r3d_posegraph_params p;
    int rc;
    if ((rc = pg_params_ok(ctx, who, params, p, n_nodes)) ||
        (rc = pg_edge_args_ok(ctx, who, n_edges, d_edge_nodes, d_edge_T, d_edge_info, d_edge_uncertain, d_edge_confidence)))
        return rc;
    if (!d_poses || (n_edges > 0 && !d_edge_kept)) return r3d_fail(ctx, R3D_E_BADARG, "%s: a missing array", who);
    R3D_HIP(ctx, hipSetDevice(ctx->device));
    DevArena ar(ctx);
    PgWork W;
    W.N = (int)n_nodes; W.E = (int)n_edges;
    W.X = d_poses; W.conf = d_edge_confidence; W.kept = d_edge_kept;
    W.nodes = d_edge_nodes; W.T = d_edge_T; W.info = d_edge_info; W.unc = d_edge_uncertain;
    W.trace = p.trace_capacity > 0 ? d_trace : nullptr;
    if ((rc = pg_run(ctx, ar, who, p, W, stats))) return rc;
    R3D_HIP(ctx, hipStreamSynchronize(ctx->stream));   // the arena may be handed to the next call
    return R3D_OK;
}

int r3d_posegraph_optimize(r3d_ctx *ctx, const r3d_posegraph_params *params, int64_t n_nodes, double *poses, int64_t n_edges, const int32_t *edge_nodes,
                           const double *edge_T, const double *edge_info, const uint8_t *edge_uncertain, double *edge_confidence, uint8_t *edge_kept,
                           r3d_posegraph_stats *stats, double *trace) {
    R3D_ROCTX_RANGE("r3d_posegraph_optimize");
    if (!ctx) return R3D_E_BADARG;
    const char *who = "posegraph_optimize";
    r3d_posegraph_params p;
    int rc;
    if ((rc = pg_params_ok(ctx, who, params, p, n_nodes)) ||
        (rc = pg_edge_args_ok(ctx, who, n_edges, edge_nodes, edge_T, edge_info, edge_uncertain, edge_confidence)))
        return rc;
    if (!poses || (n_edges > 0 && !edge_kept)) return r3d_fail(ctx, R3D_E_BADARG, "%s: a missing array", who);
    R3D_HIP(ctx, hipSetDevice(ctx->device));
    DevArena ar(ctx);
    PgWork W;
    W.N = (int)n_nodes; W.E = (int)n_edges;
    const size_t N = W.N, E = W.E;
    const double *d_X, *d_conf;
    if ((rc = r3d_upload(ctx, ar, (const double *)poses, N * 16, &d_X)) || (rc = r3d_upload(ctx, ar, edge_nodes, E * 2, &W.nodes)) ||
        (rc = r3d_upload(ctx, ar, edge_T, E * 16, &W.T)) || (rc = r3d_upload(ctx, ar, edge_info, E * 36, &W.info)) ||
        (rc = r3d_upload(ctx, ar, edge_uncertain, E, &W.unc)) || (rc = r3d_upload(ctx, ar, (const double *)edge_confidence, E, &d_conf)))
        return rc;
    W.X = (double *)d_X; W.conf = (double *)d_conf;
    W.kept = (uint8_t *)ar.get(E ? E : 1);
    const size_t cap = trace ? (size_t)p.trace_capacity : 0;
    W.trace = cap ? (double *)ar.get(cap * 4 * 8) : nullptr;
    if (ar.rc) return ar.rc;
    if (!trace) p.trace_capacity = 0;
    r3d_posegraph_stats st = {};
    if ((rc = pg_run(ctx, ar, who, p, W, &st))) return rc;
    const size_t rows = std::min(cap, (size_t)st.trials);
    if ((rc = r3d_download(ctx, poses, (const double *)W.X, N * 16)) || (rc = r3d_download(ctx, edge_confidence, (const double *)W.conf, E)) ||
        (rc = r3d_download(ctx, edge_kept, (const uint8_t *)W.kept, E)) || (rc = r3d_download(ctx, trace, (const double *)W.trace, rows * 4)))
        return rc;
    R3D_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (stats) *stats = st;
    return R3D_OK;
}

int r3d_debug_posegraph_linearize(r3d_ctx *ctx, const r3d_posegraph_params *params, int64_t n_nodes, const double *poses, int64_t n_edges,
                                  const int32_t *edge_nodes, const double *edge_T, const double *edge_info, const uint8_t *edge_uncertain,
                                  const double *edge_confidence, double *e, double *l, double *H, double *b, double *F) {
    R3D_ROCTX_RANGE("r3d_debug_posegraph_linearize");
    if (!ctx) return R3D_E_BADARG;
    const char *who = "debug_posegraph_linearize";
    r3d_posegraph_params p;
    int rc;
    if ((rc = pg_params_ok(ctx, who, params, p, n_nodes)) ||
        (rc = pg_edge_args_ok(ctx, who, n_edges, edge_nodes, edge_T, edge_info, edge_uncertain, edge_confidence)))
        return rc;
    if (!poses || n_edges < 1) return r3d_fail(ctx, R3D_E_BADARG, "%s: no poses or no edges", who);
    R3D_HIP(ctx, hipSetDevice(ctx->device));
    DevArena ar(ctx);
    PgWork W;
    W.N = (int)n_nodes; W.E = (int)n_edges; W.n = 6 * W.N;
    W.cr = pg_crit(p);
    const size_t N = W.N, E = W.E, n = W.n;
    const double *d_X, *d_conf;
    if ((rc = r3d_upload(ctx, ar, poses, N * 16, &d_X)) || (rc = r3d_upload(ctx, ar, edge_nodes, E * 2, &W.nodes)) ||
        (rc = r3d_upload(ctx, ar, edge_T, E * 16, &W.T)) || (rc = r3d_upload(ctx, ar, edge_info, E * 36, &W.info)) ||
        (rc = r3d_upload(ctx, ar, edge_uncertain, E, &W.unc)) || (rc = r3d_upload(ctx, ar, edge_confidence, E, &d_conf)))
        return rc;
    W.X = (double *)d_X; W.conf = (double *)d_conf;
    W.kept = (uint8_t *)ar.get(E);
    double *dense = (double *)ar.get(n * n * 8);
    if (ar.rc) return ar.rc;
    if ((rc = pg_alloc(ctx, ar, W, false)) || (rc = pg_validate(ctx, who, W))) return rc;
    hipStream_t s = ctx->stream;
    k_pg_keep_all<<<(W.E + 255) / 256, 256, 0, s>>>(W.E, W.kept);
    pg_linearize(ctx, W, W.X, PG_GATE_NONE);
    k_pg_begin<<<1, 256, 0, s>>>(W.E, W.n, W.H, W.b, W.q, W.kept, W.unc, W.conf, W.info, W.cr, W.st);
    k_pg_mirror<<<(unsigned)((n * n + 255) / 256), 256, 0, s>>>(W.H, dense, W.n);
    R3D_HIP(ctx, hipGetLastError());
    PgState h;
    if ((rc = pg_read_state(ctx, W.st, h))) return rc;
    if (F) *F = h.F;
    if (l) {   // the weights are the caller's own arrays read back: 1 for a certain edge, its confidence for an uncertain one
        for (size_t k = 0; k < E; k++) l[k] = edge_uncertain[k] ? edge_confidence[k] : 1.0;
    }
    if ((rc = r3d_download(ctx, e, (const double *)W.e, E * 6)) || (rc = r3d_download(ctx, H, (const double *)dense, n * n)) ||
        (rc = r3d_download(ctx, b, (const double *)W.b, n)))
        return rc;
    R3D_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return R3D_OK;
}

int r3d_debug_posegraph_solve(r3d_ctx *ctx, int32_t n, const double *A, const double *b, double lambda, double *L, double *delta, int32_t *failed_pivot) {
    R3D_ROCTX_RANGE("r3d_debug_posegraph_solve");
    if (!ctx) return R3D_E_BADARG;
    const char *who = "debug_posegraph_solve";
    if (n < 1 || n > 6 * PG_MAX_NODES || !A || !b || !failed_pivot) return r3d_fail(ctx, R3D_E_BADARG, "%s: order outside 1..%d or a missing array", who, 6 * PG_MAX_NODES);
    R3D_HIP(ctx, hipSetDevice(ctx->device));
    DevArena ar(ctx);
    const size_t nn = (size_t)n * n;
    const double *d_A, *d_b;
    int rc;
    if ((rc = r3d_upload(ctx, ar, A, nn, &d_A)) || (rc = r3d_upload(ctx, ar, b, (size_t)n, &d_b))) return rc;
    double *work = (double *)ar.get(nn * 8), *out = (double *)ar.get(nn * 8), *c = (double *)ar.get((size_t)n * 8), *y = (double *)ar.get((size_t)n * 8),
           *x = (double *)ar.get((size_t)n * 8), *xo = (double *)ar.get((size_t)n * 8), *tile = (double *)ar.get(PG_NB * PG_NB * 8);
    PgState *st = (PgState *)ar.get(sizeof(PgState));
    if (ar.rc) return ar.rc;
    hipStream_t s = ctx->stream;
    PgState init = {};
    init.fail_col = -1;
    R3D_HIP(ctx, hipMemcpyAsync(st, &init, sizeof(PgState), hipMemcpyHostToDevice, s));
    const int t16 = (n + 15) / 16;
    k_pg_form<<<dim3(t16, t16), dim3(16, 16), 0, s>>>(d_A, d_b, work, c, n, lambda, 0, st);
    pg_factor(ctx, work, n, tile, st);
    pg_substitute(ctx, work, c, y, x, n, st);
    k_pg_lower<<<(unsigned)((nn + 255) / 256), 256, 0, s>>>(work, out, n, st);
    k_pg_delta_out<<<(n + 255) / 256, 256, 0, s>>>(x, xo, n, st);
    R3D_HIP(ctx, hipGetLastError());
    int32_t fail = -1;
    R3D_HIP(ctx, hipMemcpyAsync(&fail, &st->fail_col, 4, hipMemcpyDeviceToHost, s));
    if ((rc = r3d_download(ctx, L, (const double *)out, nn)) || (rc = r3d_download(ctx, delta, (const double *)xo, (size_t)n))) return rc;
    R3D_HIP(ctx, hipStreamSynchronize(s));
    *failed_pivot = fail;
    return R3D_OK;
}

}  // extern "C"
