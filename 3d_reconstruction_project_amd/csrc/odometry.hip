// odometry.hip -- RGB-D odometry (Open3D's compute_rgbd_odometry) on the device: image pyramids, a z-buffered warp of the source
// depth into the target and a 6x6 Gauss-Newton reduction over pixels.  The contract is DESIGN.md section 4 "RGB-D odometry";
// tests/rgbd_odometry_ref.py restates it in numpy.  Every float expression below is written in the order the contract gives
// (build.sh passes -ffp-contract=off), so the planes are bit for bit the restatement's.
//
// One iteration is three launches: k_odo_corr (one thread per source pixel, a 64-bit atomicMin per surviving pixel on a
// target-sized map), k_odo_accum (one thread per target pixel, rows in float64, wave shuffle tree -> LDS in wave order -> one slab
// per workgroup, plain stores) and k_odo_step (one workgroup: slabs in a fixed order, solve6_to_matrix, T <- U T in the device state
// block).  No float atomics anywhere: the same bits on every run.  A failure sets a sticky flag in the state block that turns the
// launches still queued into no-ops; the host enqueues everything and waits once.
#include <cstring>

#include "r3d_internal.h"

namespace {

constexpr unsigned long long ODO_EMPTY = ~0ull;
enum { ODO_ITERATE_HYBRID = 0, ODO_ITERATE_COLOR = 1, ODO_NORM = 2, ODO_INFO = 3 };
template <int MODE> struct OdoNS { static constexpr int v = MODE <= ODO_ITERATE_COLOR ? 29 : MODE == ODO_NORM ? 3 : 22; };

struct OdoCam { double fx, fy, cx, cy; };

struct OdoState {
    double T[16];
    double Mk[12];        // M = K R K^-1 row by row, then k = K t: for the camera of the next k_odo_corr launch
    double s_src, s_tgt;  // 0.5 / mean intensity over the correspondences at odo_init
    double sums[29];      // of the last iteration
    double info[21];      // upper triangle, row by row
    long long n_init, n_final;
    int failed, failed_level, failed_iteration, pad;
};

// M = K R K^-1 and k = K t by explicit scalar expressions (K^-1: the closed form of a skew-free pinhole); with R = I the last
// row of M is exactly (0, 0, 1)
__host__ __device__ inline void odo_projection(const double *T, const OdoCam &c, double *Mk) {
    double A[3][3];
    for (int j = 0; j < 3; j++) {
        A[0][j] = c.fx * T[j] + c.cx * T[8 + j];
        A[1][j] = c.fy * T[4 + j] + c.cy * T[8 + j];
        A[2][j] = T[8 + j];
    }
    for (int i = 0; i < 3; i++) {
        Mk[i * 3 + 0] = A[i][0] / c.fx;
        Mk[i * 3 + 1] = A[i][1] / c.fy;
        Mk[i * 3 + 2] = (A[i][2] - (A[i][0] * c.cx) / c.fx) - (A[i][1] * c.cy) / c.fy;
    }
    Mk[9] = c.fx * T[3] + c.cx * T[11];
    Mk[10] = c.fy * T[7] + c.cy * T[11];
    Mk[11] = T[11];
}

// ---- conversion and preparation: one thread per output pixel, the 3-tap passes through registers ---------------------------------
// one pass: the three taps added in float64 in tap order, rounded once to float32
__device__ __forceinline__ float odo_tap3(double w0, float a, double w1, float b, double w2, float c) {
    return (float)((w0 * (double)a + w1 * (double)b) + w2 * (double)c);
}
__device__ __forceinline__ int odo_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

__global__ void __launch_bounds__(256) k_odo_convert(const uint16_t *__restrict__ depth, int dstride, const uint8_t *__restrict__ color, int cstride,
                                                     int cn, int bgr, float scale, float trunc, int w, int h, float *__restrict__ oi,
                                                     float *__restrict__ od) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= w || y >= h) return;
    const uint8_t *px = color + (size_t)y * cstride + (size_t)x * cn;
    float in;
    if (cn == 1) {
        in = (float)px[0] / 255.0f;
    } else {
        const float r = (float)px[bgr ? 2 : 0], g = (float)px[1], b = (float)px[bgr ? 0 : 2];
        in = ((0.2990f * r + 0.5870f * g) + 0.1140f * b) / 255.0f;
    }
    float z = (float)depth[(size_t)y * dstride + x] / scale;
    if (z > trunc) z = 0.0f;
    oi[(size_t)y * w + x] = in;
    od[(size_t)y * w + x] = z;
}

// CLIP: the depth rule of the preparation on load (NaN where z > depth_max, z < depth_min or z <= 0)
template <bool CLIP>
__device__ __forceinline__ float odo_ld(const float *__restrict__ in, int stride, int x, int y, float dmin, float dmax) {
    const float v = in[(size_t)y * stride + x];
    if (CLIP && !(v <= dmax && v >= dmin && v > 0.0f)) return __builtin_nanf("");
    return v;
}
// Gaussian3 of the pixel (x, y): horizontal pass on its three rows, then the vertical pass
template <bool CLIP>
__device__ __forceinline__ float odo_gauss3_at(const float *__restrict__ in, int stride, int w, int h, int x, int y, float dmin, float dmax) {
    const int xl = odo_clamp(x - 1, w - 1), xr = odo_clamp(x + 1, w - 1);
    float r[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const int yy = odo_clamp(y + k - 1, h - 1);
        r[k] = odo_tap3(0.25, odo_ld<CLIP>(in, stride, xl, yy, dmin, dmax), 0.5, odo_ld<CLIP>(in, stride, x, yy, dmin, dmax), 0.25,
                        odo_ld<CLIP>(in, stride, xr, yy, dmin, dmax));
    }
    return odo_tap3(0.25, r[0], 0.5, r[1], 0.25, r[2]);
}
template <bool CLIP>
__global__ void __launch_bounds__(256) k_odo_gauss3(const float *__restrict__ in, int stride, int w, int h, float dmin, float dmax,
                                                    float *__restrict__ out) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= w || y >= h) return;
    out[(size_t)y * w + x] = odo_gauss3_at<CLIP>(in, stride, w, h, x, y, dmin, dmax);
}
// level l+1 from level l (w x h, contiguous): FILTER = Downsample(Gaussian3(in)) for the intensity, plain Downsample for the depth
template <bool FILTER>
__global__ void __launch_bounds__(256) k_odo_down(const float *__restrict__ in, int w, int h, float *__restrict__ out) {
    const int w2 = w >> 1, h2 = h >> 1;
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= w2 || y >= h2) return;
    float p[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int sx = 2 * x + (k & 1), sy = 2 * y + (k >> 1);
        p[k] = FILTER ? odo_gauss3_at<false>(in, w, w, h, sx, sy, 0.0f, 0.0f) : in[(size_t)sy * w + sx];
    }
    out[(size_t)y * w2 + x] = (((p[0] + p[1]) + p[2]) + p[3]) / 4.0f;
}
// the four target gradients of a pixel in one 16-byte record: Sobel3Dx = horizontal [-1 0 1] then vertical [1 2 1], Sobel3Dy the
// transpose, on the intensity and on the depth plane (the 0 tap is multiplied like the others: a NaN under it spreads)
__device__ __forceinline__ void odo_sobel_at(const float *__restrict__ in, int w, int h, int x, int y, float *dx, float *dy) {
    const int xl = odo_clamp(x - 1, w - 1), xr = odo_clamp(x + 1, w - 1);
    float a[3], s[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float *row = in + (size_t)odo_clamp(y + k - 1, h - 1) * w;
        const float l = row[xl], c = row[x], r = row[xr];
        a[k] = odo_tap3(-1.0, l, 0.0, c, 1.0, r);
        s[k] = odo_tap3(1.0, l, 2.0, c, 1.0, r);
    }
    *dx = odo_tap3(1.0, a[0], 2.0, a[1], 1.0, a[2]);
    *dy = odo_tap3(-1.0, s[0], 0.0, s[1], 1.0, s[2]);
}
__global__ void __launch_bounds__(256) k_odo_grad(const float *__restrict__ I, const float *__restrict__ D, int w, int h, float4 *__restrict__ out) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= w || y >= h) return;
    float4 g;
    odo_sobel_at(I, w, h, x, y, &g.x, &g.y);
    odo_sobel_at(D, w, h, x, y, &g.z, &g.w);
    out[(size_t)y * w + x] = g;
}
// source points: x = (u - cx) z / fx, y = (v - cy) z / fy, z in float64, three doubles per pixel
__global__ void __launch_bounds__(256) k_odo_points(const float *__restrict__ D, int w, int h, OdoCam c, double *__restrict__ out) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= w || y >= h) return;
    const double z = (double)D[(size_t)y * w + x];
    double *o = out + ((size_t)y * w + x) * 3;
    o[0] = (((double)x - c.cx) * z) / c.fx;
    o[1] = (((double)y - c.cy) * z) / c.fy;
    o[2] = z;
}

// ---- the loop ---------------------------------------------------------------------------------------------------------------------
struct OdoInit { double T[16]; };
__global__ void k_odo_set_pose(OdoState *st, OdoInit init, OdoCam next, int reset) {
    if (threadIdx.x != 0) return;
    if (reset) {
        st->s_src = st->s_tgt = 0.0;
        for (int i = 0; i < 29; i++) st->sums[i] = 0.0;
        for (int i = 0; i < 21; i++) st->info[i] = 0.0;
        st->n_init = st->n_final = 0;
        st->failed = 0; st->failed_level = st->failed_iteration = -1; st->pad = 0;
    }
    for (int i = 0; i < 16; i++) st->T[i] = init.T[i];
    odo_projection(st->T, next, st->Mk);
}

__global__ void __launch_bounds__(256) k_odo_corr(const OdoState *__restrict__ st, const float *__restrict__ Ds, const float *__restrict__ Dt, int w,
                                                  int h, double depth_diff_max, unsigned long long *__restrict__ map) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= w * h || st->failed) return;
    const float df = Ds[i];
    if (df != df) return;
    const double d = (double)df;
    const int v = i / w, u = i - v * w;
    const double *M = st->Mk;
    const double p0 = d * ((M[0] * (double)u + M[1] * (double)v) + M[2]) + M[9];
    const double p1 = d * ((M[3] * (double)u + M[4] * (double)v) + M[5]) + M[10];
    const double z = d * ((M[6] * (double)u + M[7] * (double)v) + M[8]) + M[11];
    if (!(z > 0.0)) return;
    // u_t = (int)(p0 / z' + 0.5) truncates toward zero: a projection in (-1.5, -0.5) lands in column 0.  The range test runs on
    // the double, so the conversion never sees a value outside int.
    const double fu = p0 / z + 0.5, fv = p1 / z + 0.5;
    if (!(fu > -1.0 && fu < (double)w && fv > -1.0 && fv < (double)h)) return;
    const int t = (int)fv * w + (int)fu;
    const float dt = Dt[t];
    if (dt != dt) return;
    if (!(fabs(z - (double)dt) <= depth_diff_max)) return;
    // a positive float orders as its bits: the smallest (float)z' wins, among equal ones the smaller source index
    const unsigned long long key = ((unsigned long long)__float_as_uint((float)z) << 32) | (unsigned)i;
    atomicMin(&map[t], key);
}

struct OdoLevel {
    const float *Is, *It, *Dt;
    const float4 *grad;
    const double *pts;
    int w, h;
    OdoCam cam;
};

template <int MODE>
__global__ void __launch_bounds__(256) k_odo_accum(const OdoState *__restrict__ st, unsigned long long *__restrict__ map, OdoLevel L, double a, double b,
                                                   double *__restrict__ slabs) {
    constexpr int NS = OdoNS<MODE>::v;
    __shared__ double part[4][NS];
    if (st->failed) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    double s[NS];
#pragma unroll
    for (int k = 0; k < NS; k++) s[k] = 0.0;
    unsigned long long key = ODO_EMPTY;
    if (i < L.w * L.h) key = map[i];
    if (key != ODO_EMPTY) {
        map[i] = ODO_EMPTY;   // ready for the next k_odo_corr
        const int src = (int)(unsigned)key;
        s[0] = 1.0;
        if (MODE == ODO_NORM) {
            s[1] = (double)L.Is[src];
            s[2] = (double)L.It[i];
        } else if (MODE == ODO_INFO) {
            const int vt = i / L.w, ut = i - vt * L.w;
            const double z = (double)L.Dt[i];
            const double x = (((double)ut - L.cam.cx) * z) / L.cam.fx, y = (((double)vt - L.cam.cy) * z) / L.cam.fy;
            const double r[3][6] = {{0.0, z, -y, 1.0, 0.0, 0.0}, {-z, 0.0, x, 0.0, 1.0, 0.0}, {y, -x, 0.0, 0.0, 0.0, 1.0}};
            int q = 1;
#pragma unroll
            for (int c = 0; c < 6; c++)
#pragma unroll
                for (int e = c; e < 6; e++, q++) s[q] = (r[0][c] * r[0][e] + r[1][c] * r[1][e]) + r[2][c] * r[2][e];
        } else {
            const double *T = st->T;
            const double Px = L.pts[(size_t)src * 3], Py = L.pts[(size_t)src * 3 + 1], Pz = L.pts[(size_t)src * 3 + 2];
            const double x = ((T[0] * Px + T[1] * Py) + T[2] * Pz) + T[3];
            const double y = ((T[4] * Px + T[5] * Py) + T[6] * Pz) + T[7];
            const double z = ((T[8] * Px + T[9] * Py) + T[10] * Pz) + T[11];
            const double fx = L.cam.fx, fy = L.cam.fy;
            const float4 g4 = L.grad[i];
            const double It = st->s_tgt * (double)L.It[i], Is = st->s_src * (double)L.Is[src];
            const double r0 = a * (It - Is);
            const double gx = 0.125 * (st->s_tgt * (double)g4.x), gy = 0.125 * (st->s_tgt * (double)g4.y);
            const double c0 = (gx * fx) / z, c1 = (gy * fy) / z;
            const double c2 = -(c0 * x + c1 * y) / z;
            const double J0[6] = {a * (-z * c1 + y * c2), a * (z * c0 - x * c2), a * (-y * c0 + x * c1), a * c0, a * c1, a * c2};
            if (MODE == ODO_ITERATE_HYBRID) {
                double qx = (double)g4.z, qy = (double)g4.w;   // a NaN depth gradient counts as 0
                qx = 0.125 * (qx != qx ? 0.0 : qx);
                qy = 0.125 * (qy != qy ? 0.0 : qy);
                const double r1 = b * ((double)L.Dt[i] - z);
                const double d0 = (qx * fx) / z, d1 = (qy * fy) / z;
                const double d2 = -(d0 * x + d1 * y) / z;
                const double J1[6] = {b * ((-z * d1 + y * d2) - y), b * ((z * d0 - x * d2) + x), b * (-y * d0 + x * d1), b * d0, b * d1, b * (d2 - 1.0)};
                s[1] = r0 * r0 + r1 * r1;
                int q = 2;
#pragma unroll
                for (int c = 0; c < 6; c++)
#pragma unroll
                    for (int e = c; e < 6; e++, q++) s[q] = J0[c] * J0[e] + J1[c] * J1[e];
#pragma unroll
                for (int c = 0; c < 6; c++) s[23 + c] = J0[c] * r0 + J1[c] * r1;
            } else {
                s[1] = r0 * r0;
                int q = 2;
#pragma unroll
                for (int c = 0; c < 6; c++)
#pragma unroll
                    for (int e = c; e < 6; e++, q++) s[q] = J0[c] * J0[e];
#pragma unroll
                for (int c = 0; c < 6; c++) s[23 + c] = J0[c] * r0;
            }
        }
    }
    // across the wave by a fixed shuffle tree, across the workgroup through LDS in wave order, one slab per workgroup
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < NS; k++) {
        double x = s[k];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) x += __shfl_down(x, off, 64);
        if (lane == 0) part[wave][k] = x;
    }
    __syncthreads();
    if (threadIdx.x < NS) {
        const int k = threadIdx.x;
        slabs[(size_t)blockIdx.x * NS + k] = ((part[0][k] + part[1][k]) + part[2][k]) + part[3][k];
    }
}

// One workgroup.  The slabs come through LDS 256 at a time (coalesced loads by all threads).  A single chain of 1200 dependent
// float64 additions per slot measured 50 us at 640 x 480, so eight threads share a slot: thread (k, part) adds slot k of the blocks
// part, part + 8, ... in block order, and the eight partial sums are added in part order -- a fixed order, the same bits on every
// run.  Thread 0 then finishes the stage.  `next`: the camera of the next k_odo_corr launch, whose M and k are made here from the
// new pose.
template <int MODE>
__global__ void __launch_bounds__(256) k_odo_step(OdoState *__restrict__ st, const double *__restrict__ slabs, int nb, int level, int iteration,
                                                  double *__restrict__ trace_row, OdoCam next) {
    constexpr int NS = OdoNS<MODE>::v;
    __shared__ double stage[256 * NS];
    __shared__ double parts[NS][8];
    __shared__ double tot[NS];
    if (st->failed) return;
    const int k = (int)threadIdx.x >> 3, part = (int)threadIdx.x & 7;
    double acc = 0.0;
    for (int base = 0; base < nb; base += 256) {
        const int blocks = nb - base < 256 ? nb - base : 256;
#pragma unroll
        for (int j = 0; j < NS; j++) {
            const int e = j * 256 + (int)threadIdx.x;
            if (e < blocks * NS) stage[e] = slabs[(size_t)base * NS + e];
        }
        __syncthreads();
        if (k < NS) {
#pragma unroll 4
            for (int blk = part; blk < blocks; blk += 8) acc += stage[blk * NS + k];
        }
        __syncthreads();
    }
    if (k < NS) parts[k][part] = acc;
    __syncthreads();
    if (threadIdx.x < NS) {
        const double *p = parts[threadIdx.x];
        tot[threadIdx.x] = ((((((p[0] + p[1]) + p[2]) + p[3]) + p[4]) + p[5]) + p[6]) + p[7];
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    if (MODE == ODO_NORM) {
        st->n_init = (long long)tot[0];
        if (tot[0] == 0.0) {
            st->failed = 1; st->failed_level = 0; st->failed_iteration = -1;
            return;
        }
        st->s_src = 0.5 / (tot[1] / tot[0]);
        st->s_tgt = 0.5 / (tot[2] / tot[0]);
    } else if (MODE == ODO_INFO) {
        st->n_final = (long long)tot[0];
        for (int k = 0; k < 21; k++) st->info[k] = tot[1 + k];
        return;
    } else {
        for (int k = 0; k < 29; k++) st->sums[k] = tot[k];
        double U[16];
        const bool ok = tot[0] != 0.0 && solve6_to_matrix(tot, U);
        if (!ok) {
            st->failed = 1; st->failed_level = level; st->failed_iteration = iteration;
            return;
        }
        double Tn[12];
        for (int r = 0; r < 3; r++) {
            for (int c = 0; c < 4; c++) Tn[r * 4 + c] = (U[r * 4] * st->T[c] + U[r * 4 + 1] * st->T[4 + c]) + U[r * 4 + 2] * st->T[8 + c];
            Tn[r * 4 + 3] += U[r * 4 + 3];
        }
        for (int k = 0; k < 12; k++) st->T[k] = Tn[k];
        if (trace_row)
            for (int k = 0; k < 16; k++) trace_row[k] = st->T[k];
    }
    odo_projection(st->T, next, st->Mk);
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------
struct OdoFrame { float *I[4], *D[4]; };
struct OdoWork {
    int levels, w[4], h[4];
    OdoCam cam[4];
    OdoFrame src, tgt;
    float4 *grad[4];
    double *pts[4];
    unsigned long long *map;
    double *slabs;
    OdoState *st;
    double a, b;
    double ddm;
    int jacobian;
};

inline dim3 odo_grid(int w, int h) { return dim3((unsigned)((w + 63) / 64), (unsigned)((h + 3) / 4)); }
inline OdoLevel odo_level(const OdoWork &W, int l) {
    return OdoLevel{W.src.I[l], W.tgt.I[l], W.tgt.D[l], W.grad[l], W.pts[l], W.w[l], W.h[l], W.cam[l]};
}

int odo_params_ok(r3d_ctx *ctx, const r3d_odometry_params *p, int w, int h, int stride, double fx, double fy, const char *who) {
    if (!p) return r3d_fail(ctx, R3D_E_BADARG, "%s: params missing", who);
    if (p->levels < 1 || p->levels > 4) return r3d_fail(ctx, R3D_E_BADARG, "%s: levels %d outside 1..4", who, p->levels);
    if (w < (1 << (p->levels - 1)) || h < (1 << (p->levels - 1)) || stride < w || (int64_t)w * h > (int64_t)1 << 30)
        return r3d_fail(ctx, R3D_E_BADARG, "%s: a %d x %d image (stride %d) does not carry %d levels", who, w, h, stride, p->levels);
    for (int i = 0; i < 4; i++)
        if (p->iterations[i] < 0 || p->iterations[i] > 100000) return r3d_fail(ctx, R3D_E_BADARG, "%s: iterations[%d] = %d", who, i, p->iterations[i]);
    if (p->jacobian != R3D_ODOMETRY_HYBRID && p->jacobian != R3D_ODOMETRY_COLOR) return r3d_fail(ctx, R3D_E_BADARG, "%s: unknown jacobian %d", who, p->jacobian);
    if (!(p->depth_diff_max >= 0) || !(fx != 0) || !(fy != 0) || !std::isfinite(fx) || !std::isfinite(fy))
        return r3d_fail(ctx, R3D_E_BADARG, "%s: depth_diff_max must be >= 0, fx and fy non-zero", who);
    return R3D_OK;
}

// pyramids of both frames, target gradients, source points, then the normalisation at `init` (device planes in)
int odo_prepare(r3d_ctx *ctx, DevArena &ar, const r3d_odometry_params *p, const float *d_sI, const float *d_sD, const float *d_tI, const float *d_tD,
                int w, int h, int stride, OdoCam cam, const double *init4x4, OdoWork &W) {
    hipStream_t st = ctx->stream;
    W.levels = p->levels;
    W.ddm = p->depth_diff_max;
    W.jacobian = p->jacobian;
    W.a = p->jacobian == R3D_ODOMETRY_HYBRID ? std::sqrt(1.0 - 0.95) : 1.0;
    W.b = p->jacobian == R3D_ODOMETRY_HYBRID ? std::sqrt(0.95) : 0.0;
    for (int l = 0; l < W.levels; l++) {
        W.w[l] = w >> l;
        W.h[l] = h >> l;
        const double s = std::ldexp(1.0, -l);
        W.cam[l] = OdoCam{cam.fx * s, cam.fy * s, cam.cx * s, cam.cy * s};
        const size_t n = (size_t)W.w[l] * W.h[l];
        W.src.I[l] = (float *)ar.get(n * 4); W.src.D[l] = (float *)ar.get(n * 4);
        W.tgt.I[l] = (float *)ar.get(n * 4); W.tgt.D[l] = (float *)ar.get(n * 4);
        W.grad[l] = (float4 *)ar.get(n * 16);
        W.pts[l] = (double *)ar.get(n * 24);
    }
    const size_t n0 = (size_t)w * h, nb0 = (n0 + 255) / 256;
    W.map = (unsigned long long *)ar.get(n0 * 8);
    W.slabs = (double *)ar.get(nb0 * 29 * 8);
    W.st = (OdoState *)ar.get(sizeof(OdoState));
    if (ar.rc) return ar.rc;
    R3D_HIP(ctx, hipMemsetAsync(W.map, 0xFF, n0 * 8, st));
    const float dmin = (float)p->depth_min, dmax = (float)p->depth_max;
    for (int f = 0; f < 2; f++) {
        OdoFrame &F = f ? W.tgt : W.src;
        k_odo_gauss3<false><<<odo_grid(w, h), 256, 0, st>>>(f ? d_tI : d_sI, stride, w, h, 0.0f, 0.0f, F.I[0]);
        k_odo_gauss3<true><<<odo_grid(w, h), 256, 0, st>>>(f ? d_tD : d_sD, stride, w, h, dmin, dmax, F.D[0]);
        for (int l = 1; l < W.levels; l++) {
            k_odo_down<true><<<odo_grid(W.w[l], W.h[l]), 256, 0, st>>>(F.I[l - 1], W.w[l - 1], W.h[l - 1], F.I[l]);
            k_odo_down<false><<<odo_grid(W.w[l], W.h[l]), 256, 0, st>>>(F.D[l - 1], W.w[l - 1], W.h[l - 1], F.D[l]);
        }
    }
    for (int l = 0; l < W.levels; l++) {
        k_odo_grad<<<odo_grid(W.w[l], W.h[l]), 256, 0, st>>>(W.tgt.I[l], W.tgt.D[l], W.w[l], W.h[l], W.grad[l]);
        k_odo_points<<<odo_grid(W.w[l], W.h[l]), 256, 0, st>>>(W.src.D[l], W.w[l], W.h[l], W.cam[l], W.pts[l]);
    }
    OdoInit init;
    for (int i = 0; i < 16; i++) init.T[i] = init4x4 ? init4x4[i] : (double)(i % 5 == 0);
    k_odo_set_pose<<<1, 64, 0, st>>>(W.st, init, W.cam[0], 1);
    k_odo_corr<<<(unsigned)nb0, 256, 0, st>>>(W.st, W.src.D[0], W.tgt.D[0], w, h, W.ddm, W.map);
    k_odo_accum<ODO_NORM><<<(unsigned)nb0, 256, 0, st>>>(W.st, W.map, odo_level(W, 0), W.a, W.b, W.slabs);
    return R3D_OK;   // the caller launches k_odo_step<ODO_NORM> with the camera of its next stage
}

int odo_iteration(r3d_ctx *ctx, const OdoWork &W, int l, int it, double *trace_row, OdoCam next) {
    hipStream_t st = ctx->stream;
    const unsigned nb = (unsigned)(((size_t)W.w[l] * W.h[l] + 255) / 256);
    k_odo_corr<<<nb, 256, 0, st>>>(W.st, W.src.D[l], W.tgt.D[l], W.w[l], W.h[l], W.ddm, W.map);
    if (W.jacobian == R3D_ODOMETRY_HYBRID) {
        k_odo_accum<ODO_ITERATE_HYBRID><<<nb, 256, 0, st>>>(W.st, W.map, odo_level(W, l), W.a, W.b, W.slabs);
        k_odo_step<ODO_ITERATE_HYBRID><<<1, 256, 0, st>>>(W.st, W.slabs, (int)nb, l, it, trace_row, next);
    } else {
        k_odo_accum<ODO_ITERATE_COLOR><<<nb, 256, 0, st>>>(W.st, W.map, odo_level(W, l), W.a, W.b, W.slabs);
        k_odo_step<ODO_ITERATE_COLOR><<<1, 256, 0, st>>>(W.st, W.slabs, (int)nb, l, it, trace_row, next);
    }
    R3D_HIP(ctx, hipGetLastError());
    return R3D_OK;
}

// the whole call on device planes
int odo_run(r3d_ctx *ctx, DevArena &ar, const r3d_odometry_params *p, const float *d_sI, const float *d_sD, const float *d_tI, const float *d_tD, int w,
            int h, int stride, OdoCam cam, const double *init4x4, double *T4x4, double *info6x6, r3d_odometry_stats *stats, double *trace_T) {
    hipStream_t st = ctx->stream;
    r3d_events<3> ev;
    R3D_HIP(ctx, ev.create_all());
    R3D_HIP(ctx, hipEventRecord(ev[0], st));
    OdoWork W;
    int rc;
    if ((rc = odo_prepare(ctx, ar, p, d_sI, d_sD, d_tI, d_tD, w, h, stride, cam, init4x4, W))) return rc;
    int total = 0, first = -1;   // first: the level of the first iteration
    for (int k = 0; k < W.levels; k++) {
        total += p->iterations[k];
        if (first < 0 && p->iterations[k] > 0) first = W.levels - 1 - k;
    }
    double *d_trace = nullptr;
    if (trace_T && total > 0) {
        d_trace = (double *)ar.get((size_t)total * 128);
        if (ar.rc) return ar.rc;
        R3D_HIP(ctx, hipMemsetAsync(d_trace, 0, (size_t)total * 128, st));
    }
    const unsigned nb0 = (unsigned)(((size_t)w * h + 255) / 256);
    k_odo_step<ODO_NORM><<<1, 256, 0, st>>>(W.st, W.slabs, (int)nb0, 0, -1, nullptr, W.cam[first < 0 ? 0 : first]);
    R3D_HIP(ctx, hipGetLastError());
    R3D_HIP(ctx, hipEventRecord(ev[1], st));
    int done = 0;
    for (int k = 0; k < W.levels; k++) {
        const int l = W.levels - 1 - k;
        for (int it = 0; it < p->iterations[k]; it++, done++) {
            // the camera of the launch after this step: this level again, the next level that iterates, or level 0 for the information matrix
            int nl = l;
            if (it + 1 == p->iterations[k]) {
                nl = 0;
                for (int k2 = k + 1; k2 < W.levels; k2++)
                    if (p->iterations[k2] > 0) { nl = W.levels - 1 - k2; break; }
            }
            if ((rc = odo_iteration(ctx, W, l, it, d_trace ? d_trace + (size_t)done * 16 : nullptr, W.cam[nl]))) return rc;
        }
    }
    k_odo_corr<<<nb0, 256, 0, st>>>(W.st, W.src.D[0], W.tgt.D[0], w, h, W.ddm, W.map);
    k_odo_accum<ODO_INFO><<<nb0, 256, 0, st>>>(W.st, W.map, odo_level(W, 0), W.a, W.b, W.slabs);
    k_odo_step<ODO_INFO><<<1, 256, 0, st>>>(W.st, W.slabs, (int)nb0, 0, -1, nullptr, W.cam[0]);
    R3D_HIP(ctx, hipGetLastError());
    R3D_HIP(ctx, hipEventRecord(ev[2], st));
    OdoState hs;
    R3D_HIP(ctx, hipMemcpyAsync(&hs, W.st, sizeof(hs), hipMemcpyDeviceToHost, st));
    if (d_trace && (rc = r3d_download(ctx, trace_T, d_trace, (size_t)total * 16))) return rc;
    R3D_HIP(ctx, hipStreamSynchronize(st));   // the one wait of the call
    const bool ok = !hs.failed;
    for (int i = 0; i < 16; i++) T4x4[i] = ok ? hs.T[i] : (double)(i % 5 == 0);
    if (info6x6) {
        for (int i = 0; i < 36; i++) info6x6[i] = ok ? 0.0 : (double)(i % 7 == 0);
        if (ok)
            for (int c = 0, q = 0; c < 6; c++)
                for (int e = c; e < 6; e++, q++) info6x6[c * 6 + e] = info6x6[e * 6 + c] = hs.info[q];
    }
    if (stats) {
        memset(stats, 0, sizeof(*stats));
        stats->success = ok;
        stats->failed_level = ok ? -1 : hs.failed_level;
        stats->failed_iteration = ok ? -1 : hs.failed_iteration;
        stats->correspondences_init = hs.n_init;
        stats->correspondences = ok ? hs.n_final : 0;
        stats->r2 = ok ? hs.sums[1] : 0.0;
        float ms = 0;
        R3D_HIP(ctx, hipEventElapsedTime(&ms, ev[0], ev[1]));
        stats->setup_ms = ms;
        R3D_HIP(ctx, hipEventElapsedTime(&ms, ev[1], ev[2]));
        stats->loop_ms = ms;
    }
    return R3D_OK;
}

int odo_convert(r3d_ctx *ctx, DevArena &ar, const uint16_t *depth, const uint8_t *color, int w, int h, int dstride, int cstride, int cn, int bgr,
                const r3d_depth_camera *cam, float **d_I, float **d_D) {
    uint16_t *dd;
    uint8_t *dc;
    int rc;
    if ((rc = r3d_upload_plane(ctx, ar, depth, w, h, dstride, &dd)) || (rc = r3d_upload_plane(ctx, ar, color, w * cn, h, cstride, &dc))) return rc;
    *d_I = (float *)ar.get((size_t)w * h * 4);
    *d_D = (float *)ar.get((size_t)w * h * 4);
    if (ar.rc) return ar.rc;
    k_odo_convert<<<odo_grid(w, h), 256, 0, ctx->stream>>>(dd, w, dc, w * cn, cn, bgr, (float)cam->depth_scale, (float)cam->depth_trunc, w, h, *d_I, *d_D);
    R3D_HIP(ctx, hipGetLastError());
    return R3D_OK;
}

int odo_raw_ok(r3d_ctx *ctx, const uint16_t *depth, const uint8_t *color, int w, int h, int dstride, int cstride, int cn, const r3d_depth_camera *cam,
               const char *who) {
    if (!depth || !color || !cam || w <= 0 || h <= 0 || (cn != 1 && cn != 3) || dstride < w || (int64_t)cstride < (int64_t)w * cn)
        return r3d_fail(ctx, R3D_E_BADARG, "%s: a missing image, color_channels other than 1 or 3, or a stride too small", who);
    if (!(cam->fx != 0) || !(cam->fy != 0) || !(cam->depth_scale > 0) || !(cam->depth_trunc > 0))
        return r3d_fail(ctx, R3D_E_BADARG, "%s: focal lengths must be non-zero, depth_scale and depth_trunc positive", who);
    return R3D_OK;
}

}  // namespace

extern "C" {

int r3d_rgbd_odometry_f32_dev(r3d_ctx *ctx, const r3d_odometry_params *p, const float *d_src_intensity, const float *d_src_depth,
                              const float *d_tgt_intensity, const float *d_tgt_depth, int32_t w, int32_t h, int32_t stride, double fx, double fy,
                              double cx, double cy, const double *init4x4, double *T4x4, double *info6x6, r3d_odometry_stats *stats, double *trace_T) {
    R3D_ROCTX_RANGE("r3d_rgbd_odometry_f32_dev");
    if (!ctx) return R3D_E_BADARG;
    if (!d_src_intensity || !d_src_depth || !d_tgt_intensity || !d_tgt_depth || !T4x4) return r3d_fail(ctx, R3D_E_BADARG, "rgbd_odometry: a missing array");
    int rc;
    if ((rc = odo_params_ok(ctx, p, w, h, stride, fx, fy, "rgbd_odometry"))) return rc;
    R3D_HIP(ctx, hipSetDevice(ctx->device));
    DevArena ar(ctx);
    return odo_run(ctx, ar, p, d_src_intensity, d_src_depth, d_tgt_intensity, d_tgt_depth, w, h, stride, OdoCam{fx, fy, cx, cy}, init4x4, T4x4, info6x6,
                   stats, trace_T);
}

int r3d_rgbd_odometry_f32(r3d_ctx *ctx, const r3d_odometry_params *p, const float *src_intensity, const float *src_depth, const float *tgt_intensity,
                          const float *tgt_depth, int32_t w, int32_t h, int32_t stride, double fx, double fy, double cx, double cy,
                          const double *init4x4, double *T4x4, double *info6x6, r3d_odometry_stats *stats, double *trace_T) {
    R3D_ROCTX_RANGE("r3d_rgbd_odometry_f32");
    if (!ctx) return R3D_E_BADARG;
    if (!src_intensity || !src_depth || !tgt_intensity || !tgt_depth || !T4x4) return r3d_fail(ctx, R3D_E_BADARG, "rgbd_odometry: a missing array");
    int rc;
    if ((rc = odo_params_ok(ctx, p, w, h, stride, fx, fy, "rgbd_odometry"))) return rc;
    R3D_HIP(ctx, hipSetDevice(ctx->device));
    DevArena ar(ctx);
    const float *const host[4] = {src_intensity, src_depth, tgt_intensity, tgt_depth};
    float *dev[4];
    for (int k = 0; k < 4; k++) if ((rc = r3d_upload_plane(ctx, ar, host[k], w, h, stride, &dev[k]))) return rc;   // -> dense device planes
    return odo_run(ctx, ar, p, dev[0], dev[1], dev[2], dev[3], w, h, w, OdoCam{fx, fy, cx, cy}, init4x4, T4x4, info6x6, stats, trace_T);
}

int r3d_rgbd_odometry(r3d_ctx *ctx, const r3d_odometry_params *p, const uint16_t *src_depth, const uint8_t *src_color, const uint16_t *tgt_depth,
                      const uint8_t *tgt_color, int32_t w, int32_t h, int32_t depth_stride, int32_t color_stride, int32_t color_channels,
                      int32_t color_bgr, const r3d_depth_camera *cam, const double *init4x4, double *T4x4, double *info6x6, r3d_odometry_stats *stats,
                      double *trace_T) {
    R3D_ROCTX_RANGE("r3d_rgbd_odometry");
    if (!ctx) return R3D_E_BADARG;
    if (!T4x4) return r3d_fail(ctx, R3D_E_BADARG, "rgbd_odometry: a missing array");
    int rc;
    if ((rc = odo_raw_ok(ctx, src_depth, src_color, w, h, depth_stride, color_stride, color_channels, cam, "rgbd_odometry"))) return rc;
    if ((rc = odo_raw_ok(ctx, tgt_depth, tgt_color, w, h, depth_stride, color_stride, color_channels, cam, "rgbd_odometry"))) return rc;
    if ((rc = odo_params_ok(ctx, p, w, h, w, cam->fx, cam->fy, "rgbd_odometry"))) return rc;
    R3D_HIP(ctx, hipSetDevice(ctx->device));
    DevArena ar(ctx);
    float *sI, *sD, *tI, *tD;
    if ((rc = odo_convert(ctx, ar, src_depth, src_color, w, h, depth_stride, color_stride, color_channels, color_bgr, cam, &sI, &sD))) return rc;
    if ((rc = odo_convert(ctx, ar, tgt_depth, tgt_color, w, h, depth_stride, color_stride, color_channels, color_bgr, cam, &tI, &tD))) return rc;
    return odo_run(ctx, ar, p, sI, sD, tI, tD, w, h, w, OdoCam{cam->fx, cam->fy, cam->ppx, cam->ppy}, init4x4, T4x4, info6x6, stats, trace_T);
}

int r3d_debug_rgbd_convert(r3d_ctx *ctx, const uint16_t *depth, const uint8_t *color, int32_t w, int32_t h, int32_t depth_stride, int32_t color_stride,
                           int32_t color_channels, int32_t color_bgr, const r3d_depth_camera *cam, float *out_intensity, float *out_depth) {
    R3D_ROCTX_RANGE("r3d_debug_rgbd_convert");
    if (!ctx) return R3D_E_BADARG;
    if (!out_intensity || !out_depth) return r3d_fail(ctx, R3D_E_BADARG, "debug_rgbd_convert: a missing array");
    int rc;
    if ((rc = odo_raw_ok(ctx, depth, color, w, h, depth_stride, color_stride, color_channels, cam, "debug_rgbd_convert"))) return rc;
    R3D_HIP(ctx, hipSetDevice(ctx->device));
    DevArena ar(ctx);
    float *dI, *dD;
    if ((rc = odo_convert(ctx, ar, depth, color, w, h, depth_stride, color_stride, color_channels, color_bgr, cam, &dI, &dD))) return rc;
    if ((rc = r3d_download(ctx, out_intensity, dI, (size_t)w * h)) || (rc = r3d_download(ctx, out_depth, dD, (size_t)w * h))) return rc;
    R3D_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return R3D_OK;
}

int r3d_debug_rgbd_prepare(r3d_ctx *ctx, const r3d_odometry_params *p, const float *src_intensity, const float *src_depth, const float *tgt_intensity,
                           const float *tgt_depth, int32_t w, int32_t h, int32_t stride, double fx, double fy, double cx, double cy,
                           const double *init4x4, float *src_pyr_intensity, float *src_pyr_depth, float *tgt_pyr_intensity, float *tgt_pyr_depth,
                           int32_t grad_level, float *grad4, int64_t *corr_init, double *scales2) {
    R3D_ROCTX_RANGE("r3d_debug_rgbd_prepare");
    if (!ctx) return R3D_E_BADARG;
    if (!src_intensity || !src_depth || !tgt_intensity || !tgt_depth) return r3d_fail(ctx, R3D_E_BADARG, "debug_rgbd_prepare: a missing array");
    int rc;
    if ((rc = odo_params_ok(ctx, p, w, h, stride, fx, fy, "debug_rgbd_prepare"))) return rc;
    if (grad4 && (grad_level < 0 || grad_level >= p->levels)) return r3d_fail(ctx, R3D_E_BADARG, "debug_rgbd_prepare: grad_level %d", grad_level);
    R3D_HIP(ctx, hipSetDevice(ctx->device));
    DevArena ar(ctx);
    const float *const host[4] = {src_intensity, src_depth, tgt_intensity, tgt_depth};
    float *dev[4];
    for (int k = 0; k < 4; k++) if ((rc = r3d_upload_plane(ctx, ar, host[k], w, h, stride, &dev[k]))) return rc;   // -> dense device planes
    OdoWork W;
    if ((rc = odo_prepare(ctx, ar, p, dev[0], dev[1], dev[2], dev[3], w, h, w, OdoCam{fx, fy, cx, cy}, init4x4, W))) return rc;
    hipStream_t st = ctx->stream;
    k_odo_step<ODO_NORM><<<1, 256, 0, st>>>(W.st, W.slabs, (int)(((size_t)w * h + 255) / 256), 0, -1, nullptr, W.cam[0]);
    R3D_HIP(ctx, hipGetLastError());
    float *outs[4] = {src_pyr_intensity, src_pyr_depth, tgt_pyr_intensity, tgt_pyr_depth};
    size_t off = 0;
    for (int l = 0; l < W.levels; l++) {
        const size_t n = (size_t)W.w[l] * W.h[l];
        const float *planes[4] = {W.src.I[l], W.src.D[l], W.tgt.I[l], W.tgt.D[l]};
        for (int k = 0; k < 4; k++)
            if (outs[k] && (rc = r3d_download(ctx, outs[k] + off, planes[k], n))) return rc;
        off += n;
    }
    if (grad4 && (rc = r3d_download(ctx, grad4, (const float *)W.grad[grad_level], (size_t)W.w[grad_level] * W.h[grad_level] * 4))) return rc;
    OdoState hs;
    R3D_HIP(ctx, hipMemcpyAsync(&hs, W.st, sizeof(hs), hipMemcpyDeviceToHost, st));
    R3D_HIP(ctx, hipStreamSynchronize(st));
    if (corr_init) *corr_init = hs.n_init;
    if (scales2) { scales2[0] = hs.s_src; scales2[1] = hs.s_tgt; }
    return R3D_OK;
}

int r3d_debug_rgbd_iteration(r3d_ctx *ctx, const r3d_odometry_params *p, const float *src_intensity, const float *src_depth, const float *tgt_intensity,
                             const float *tgt_depth, int32_t w, int32_t h, int32_t stride, double fx, double fy, double cx, double cy,
                             const double *init4x4, int32_t level, const double *pose4x4, int32_t *corr, int64_t *n_corr, double *sums29,
                             double *T_after, int32_t *ok) {
    R3D_ROCTX_RANGE("r3d_debug_rgbd_iteration");
    if (!ctx) return R3D_E_BADARG;
    if (!src_intensity || !src_depth || !tgt_intensity || !tgt_depth || !pose4x4 || !n_corr || !sums29 || !T_after || !ok)
        return r3d_fail(ctx, R3D_E_BADARG, "debug_rgbd_iteration: a missing array");
    int rc;
    if ((rc = odo_params_ok(ctx, p, w, h, stride, fx, fy, "debug_rgbd_iteration"))) return rc;
    if (level < 0 || level >= p->levels) return r3d_fail(ctx, R3D_E_BADARG, "debug_rgbd_iteration: level %d outside 0..%d", level, p->levels - 1);
    R3D_HIP(ctx, hipSetDevice(ctx->device));
    DevArena ar(ctx);
    const float *const host[4] = {src_intensity, src_depth, tgt_intensity, tgt_depth};
    float *dev[4];
    for (int k = 0; k < 4; k++) if ((rc = r3d_upload_plane(ctx, ar, host[k], w, h, stride, &dev[k]))) return rc;   // -> dense device planes
    OdoWork W;
    if ((rc = odo_prepare(ctx, ar, p, dev[0], dev[1], dev[2], dev[3], w, h, w, OdoCam{fx, fy, cx, cy}, init4x4, W))) return rc;
    hipStream_t st = ctx->stream;
    k_odo_step<ODO_NORM><<<1, 256, 0, st>>>(W.st, W.slabs, (int)(((size_t)w * h + 255) / 256), 0, -1, nullptr, W.cam[level]);
    OdoInit pose;
    for (int i = 0; i < 16; i++) pose.T[i] = pose4x4[i];
    k_odo_set_pose<<<1, 64, 0, st>>>(W.st, pose, W.cam[level], 0);
    const int wl = W.w[level], hl = W.h[level];
    const size_t nl = (size_t)wl * hl;
    const unsigned nb = (unsigned)((nl + 255) / 256);
    k_odo_corr<<<nb, 256, 0, st>>>(W.st, W.src.D[level], W.tgt.D[level], wl, hl, W.ddm, W.map);
    R3D_HIP(ctx, hipGetLastError());
    std::vector<unsigned long long> hmap(nl);
    R3D_HIP(ctx, hipMemcpyAsync(hmap.data(), W.map, nl * 8, hipMemcpyDeviceToHost, st));   // before k_odo_accum resets the map
    R3D_HIP(ctx, hipStreamSynchronize(st));
    if ((rc = odo_iteration(ctx, W, level, 0, nullptr, W.cam[level]))) return rc;
    OdoState hs;
    R3D_HIP(ctx, hipMemcpyAsync(&hs, W.st, sizeof(hs), hipMemcpyDeviceToHost, st));
    R3D_HIP(ctx, hipStreamSynchronize(st));
    if (hs.failed && hs.failed_iteration < 0) return r3d_fail(ctx, R3D_E_BADARG, "debug_rgbd_iteration: no correspondences at init4x4");
    int64_t n = 0;
    for (size_t t = 0; t < nl; t++) {
        if (hmap[t] == ODO_EMPTY) continue;
        if (corr) {
            const int s = (int)(unsigned)hmap[t];
            corr[n * 4] = s % wl; corr[n * 4 + 1] = s / wl; corr[n * 4 + 2] = (int)(t % wl); corr[n * 4 + 3] = (int)(t / wl);
        }
        n++;
    }
    *n_corr = n;
    *ok = !hs.failed;
    for (int i = 0; i < 29; i++) sums29[i] = hs.sums[i];
    for (int i = 0; i < 16; i++) T_after[i] = hs.failed ? (double)(i % 5 == 0) : hs.T[i];
    return R3D_OK;
}

}  // extern "C"
