// tsdf.hip -- Open3D's ScalableTSDFVolume on the device: posed RGB-D frames are integrated into a sparse volume of 16^3-voxel units
// and a point cloud is extracted from it.  The contract is DESIGN.md section 4 "TSDF volume"; tests/tsdf_ref.py restates it in
// numpy.  Every float expression below is written in the order the contract gives (build.sh passes -ffp-contract=off), so the
// planes, the points and the colours are bit for bit the restatement's.
//
// A volume owns an open-addressing hash table of packed unit keys and a pool of unit blocks kept as planes (tsdf, weight, three
// colour planes; 4096 entries per unit, the z walk of one (x, y) column contiguous).  One frame is three launches: k_tsdf_touch
// (one thread per sampled pixel inserts the box of units around its point, lists the table entries that are new and those seen
// for the first time in this frame), k_tsdf_assign (new entries get the next pool slots) and k_tsdf_integrate (one workgroup
// per touched unit, one thread per column).  Between touch and assign the host reads 16 bytes of counters: how many units are new
// decides whether pool and table must grow first.  Which slot a unit gets depends on which thread won the race; nothing
// observable does: extraction and the debug dump walk the units in key order.  No kernel waits for another workgroup.
#include <algorithm>
#include <cstring>
#include <vector>

#include "r3d_internal.h"
#include "tsdf_mc_tables.h"

namespace {

constexpr int TSDF_R = 16;                    // volume_unit_resolution (the only one)
constexpr int TSDF_UNIT = TSDF_R * TSDF_R * TSDF_R;
constexpr int TSDF_IDX_LIMIT = 1 << 20;       // unit indices in [-2^20, 2^20): 21 bits per axis
constexpr unsigned long long TSDF_EMPTY = ~0ull;
constexpr int TSDF_DEFAULT_UNITS = 1024;

struct TsdfCounters { int n_new, n_touched, table_full, out_of_range; };

struct TsdfTable {
    unsigned long long *keys;   // TSDF_EMPTY or a packed unit key
    int *slot;                  // pool slot of the entry's unit
    int *stamp;                 // number of the touch pass that last saw the entry
    int cap;                    // a power of two, at least twice the pool capacity
};

struct TsdfCam { double fx, fy, cx, cy; };
struct TsdfPose { double Ai[9], ti[3]; };   // camera -> world: the inverse of the extrinsic

// key order = ascending (X, Y, Z)
__host__ __device__ inline unsigned long long tsdf_pack(int X, int Y, int Z) {
    return ((unsigned long long)(X + TSDF_IDX_LIMIT) << 42) | ((unsigned long long)(Y + TSDF_IDX_LIMIT) << 21) |
           (unsigned long long)(Z + TSDF_IDX_LIMIT);
}
__host__ __device__ inline void tsdf_unpack(unsigned long long key, int &X, int &Y, int &Z) {
    X = (int)(key >> 42) - TSDF_IDX_LIMIT;
    Y = (int)((key >> 21) & 0x1FFFFF) - TSDF_IDX_LIMIT;
    Z = (int)(key & 0x1FFFFF) - TSDF_IDX_LIMIT;
}
__device__ __forceinline__ bool tsdf_in_range(int X, int Y, int Z) {
    return X >= -TSDF_IDX_LIMIT && X < TSDF_IDX_LIMIT && Y >= -TSDF_IDX_LIMIT && Y < TSDF_IDX_LIMIT && Z >= -TSDF_IDX_LIMIT && Z < TSDF_IDX_LIMIT;
}
__device__ __forceinline__ unsigned tsdf_hash(unsigned long long k) {
    k ^= k >> 33; k *= 0xff51afd7ed558ccdULL; k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ULL; k ^= k >> 33;
    return (unsigned)k;
}
// pool slot of the unit (X, Y, Z), -1 when the volume has no such unit
__device__ inline int tsdf_find(const TsdfTable &t, int X, int Y, int Z) {
    if (!tsdf_in_range(X, Y, Z)) return -1;
    const unsigned long long key = tsdf_pack(X, Y, Z);
    const unsigned mask = (unsigned)t.cap - 1u;
    unsigned h = tsdf_hash(key) & mask;
    for (int probe = 0; probe < t.cap; probe++, h = (h + 1u) & mask) {
        const unsigned long long k = t.keys[h];
        if (k == key) return t.slot[h];
        if (k == TSDF_EMPTY) return -1;
    }
    return -1;
}

__global__ void __launch_bounds__(256) k_tsdf_depth_u16(const uint16_t *__restrict__ raw, int w, int h, float scale, float trunc, float *__restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= w * h) return;
    float z = (float)raw[i] / scale;
    if (z > trunc) z = 0.0f;
    out[i] = z;
}

// ---- touch ------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_tsdf_touch(const float *__restrict__ depth, int dstride, int s, int nj, int ni, TsdfCam c, TsdfPose P,
                                                    double trunc, double ul, TsdfTable t, int pass, int *__restrict__ new_list,
                                                    int *__restrict__ touched, TsdfCounters *__restrict__ cnt) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= ni * nj) return;
    const int i = (idx / nj) * s, j = (idx % nj) * s;
    const float zf = depth[(size_t)i * dstride + j];
    if (!(zf > 0.0f)) return;
    const double z = (double)zf;
    const double x = (((double)j - c.cx) * z) / c.fx, y = (((double)i - c.cy) * z) / c.fy;
    int lo[3], hi[3];
    for (int k = 0; k < 3; k++) {
        const double p = ((P.Ai[k * 3] * x + P.Ai[k * 3 + 1] * y) + P.Ai[k * 3 + 2] * z) + P.ti[k];
        const double l = floor((p - trunc) / ul), u = floor((p + trunc) / ul);
        if (!(l >= (double)-TSDF_IDX_LIMIT && u < (double)TSDF_IDX_LIMIT)) {   // also a NaN or an infinity
            cnt->out_of_range = 1;
            return;
        }
        lo[k] = (int)l;
        hi[k] = (int)u;
    }
    const unsigned mask = (unsigned)t.cap - 1u;
    for (int X = lo[0]; X <= hi[0]; X++)
        for (int Y = lo[1]; Y <= hi[1]; Y++)
            for (int Z = lo[2]; Z <= hi[2]; Z++) {
                const unsigned long long key = tsdf_pack(X, Y, Z);
                unsigned h = tsdf_hash(key) & mask;
                bool placed = false;
                for (int probe = 0; probe < t.cap; probe++, h = (h + 1u) & mask) {
                    unsigned long long k = t.keys[h];
                    if (k == TSDF_EMPTY) {
                        k = atomicCAS(&t.keys[h], TSDF_EMPTY, key);
                        if (k == TSDF_EMPTY) {
                            new_list[atomicAdd(&cnt->n_new, 1)] = (int)h;   // at most t.cap entries can be claimed
                            k = key;
                        }
                    }
                    if (k == key) {
                        if (atomicExch(&t.stamp[h], pass) != pass) touched[atomicAdd(&cnt->n_touched, 1)] = (int)h;
                        placed = true;
                        break;
                    }
                }
                if (!placed) {
                    cnt->table_full = 1;
                    return;
                }
            }
}

__global__ void __launch_bounds__(256) k_tsdf_assign(TsdfTable t, const int *__restrict__ new_list, int n_new, int base,
                                                     unsigned long long *__restrict__ unit_keys) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_new) return;
    const int h = new_list[i];
    t.slot[h] = base + i;
    unit_keys[base + i] = t.keys[h];
}

// the table from the units alone (after a growth, and to forget the entries of a touch pass that was given up)
__global__ void __launch_bounds__(256) k_tsdf_rebuild(TsdfTable t, const unsigned long long *__restrict__ unit_keys, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const unsigned long long key = unit_keys[i];
    const unsigned mask = (unsigned)t.cap - 1u;
    unsigned h = tsdf_hash(key) & mask;
    for (int probe = 0; probe < t.cap; probe++, h = (h + 1u) & mask)
        if (atomicCAS(&t.keys[h], TSDF_EMPTY, key) == TSDF_EMPTY) {
            t.slot[h] = i;
            return;
        }
}

// ---- integrate --------------------------------------------------------------------------------------------------------------------
struct TsdfFrame {
    const float *depth;
    const uint8_t *color;
    int dstride, cstride, w, h;
    float fx, fy, cx, cy, ifx, ify;   // ifx = 1.0f / fx
    float E[12];                      // float32 of the extrinsic's first three rows
    float vl, trunc, itrunc, wlim, hlim;
    double vld, ul;
};

// QUIRK_TSDF_MATVEC_ORDER: ((E0 x + E1 y) + E2 z) + E3.  QUIRK_TSDF_Z_RUNNING_SUM: the camera point of z + 1 is that of z plus
// f32(E[k][2] * f32(vl)), a running float32 sum down the column.
template <bool COLOR>
__global__ void __launch_bounds__(256) k_tsdf_integrate(TsdfFrame F, TsdfTable t, const int *__restrict__ touched, float *__restrict__ tsdf,
                                                        float *__restrict__ weight, double *__restrict__ c0, double *__restrict__ c1,
                                                        double *__restrict__ c2) {
    const int h = touched[blockIdx.x];
    const int slot = t.slot[h];
    int X, Y, Z;
    tsdf_unpack(t.keys[h], X, Y, Z);
    const int x = (int)threadIdx.x >> 4, y = (int)threadIdx.x & 15;
    const double half = 0.5 * F.vld;
    const float Px = (float)((half + F.vld * (double)x) + (double)X * F.ul);
    const float Py = (float)((half + F.vld * (double)y) + (double)Y * F.ul);
    const float Pz = (float)(half + (double)Z * F.ul);
    float pc0 = ((F.E[0] * Px + F.E[1] * Py) + F.E[2] * Pz) + F.E[3];
    float pc1 = ((F.E[4] * Px + F.E[5] * Py) + F.E[6] * Pz) + F.E[7];
    float pc2 = ((F.E[8] * Px + F.E[9] * Py) + F.E[10] * Pz) + F.E[11];
    const float s0 = F.E[2] * F.vl, s1 = F.E[6] * F.vl, s2 = F.E[10] * F.vl;
    // first the walk alone: which voxels of the column update, with what value, from which pixel.  A column with none (most of
    // them: outside the image, on a hole, far behind the surface) loads and stores nothing.  The 16 values and pixel offsets of
    // a thread wait in LDS (its own entries, [z][thread]: no bank conflict, no barrier): held in registers, the unrolled walk
    // took all 256 VGPRs and left one wave per SIMD.
    __shared__ float s_tv[TSDF_R * 256];
    __shared__ int s_pix[COLOR ? TSDF_R * 256 : 1];
    const int tid = (int)threadIdx.x;
    unsigned upd = 0;
#pragma unroll 2
    for (int z = 0; z < TSDF_R; z++) {
        if (pc2 > 0.0f) {
            const float uf = ((pc0 * F.fx) / pc2 + F.cx) + 0.5f, vf = ((pc1 * F.fy) / pc2 + F.cy) + 0.5f;
            if (uf >= 0.0001f && uf < F.wlim && vf >= 0.0001f && vf < F.hlim) {
                int u = (int)uf, v = (int)vf;
                u = u < F.w ? u : F.w - 1;   // never taken while wlim < w; keeps the gather inside the image whatever wlim rounds to
                v = v < F.h ? v : F.h - 1;
                const float d = F.depth[(size_t)v * F.dstride + u];
                if (d > 0.0f) {
                    const float xx = ((float)u - F.cx) * F.ifx, yy = ((float)v - F.cy) * F.ify;
                    const float mult = sqrtf((xx * xx + yy * yy) + 1.0f);
                    const float sdf = (d - pc2) * mult;
                    if (sdf > -F.trunc) {
                        const float q = sdf * F.itrunc;
                        s_tv[z * 256 + tid] = q < 1.0f ? q : 1.0f;
                        if (COLOR) s_pix[z * 256 + tid] = v * F.cstride + u * 3;
                        upd |= 1u << z;
                    }
                }
            }
        }
        pc0 += s0;
        pc1 += s1;
        pc2 += s2;
    }
    if (!upd) return;
    const size_t base = (size_t)slot * TSDF_UNIT + (size_t)threadIdx.x * TSDF_R;
    float f[TSDF_R], w[TSDF_R];
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const float4 a = reinterpret_cast<const float4 *>(tsdf + base)[q], b = reinterpret_cast<const float4 *>(weight + base)[q];
        f[q * 4] = a.x; f[q * 4 + 1] = a.y; f[q * 4 + 2] = a.z; f[q * 4 + 3] = a.w;
        w[q * 4] = b.x; w[q * 4 + 1] = b.y; w[q * 4 + 2] = b.z; w[q * 4 + 3] = b.w;
    }
    if (COLOR) {
        double *const planes[3] = {c0, c1, c2};
#pragma unroll
        for (int ch = 0; ch < 3; ch++) {
            double2 *col = reinterpret_cast<double2 *>(planes[ch] + base);
#pragma unroll
            for (int q = 0; q < 8; q++) {
                if (!((upd >> (2 * q)) & 3u)) continue;
                double2 cc = col[q];
                if ((upd >> (2 * q)) & 1u)
                    cc.x = (cc.x * (double)w[2 * q] + (double)F.color[s_pix[2 * q * 256 + tid] + ch]) / ((double)w[2 * q] + 1.0);
                if ((upd >> (2 * q + 1)) & 1u)
                    cc.y = (cc.y * (double)w[2 * q + 1] + (double)F.color[s_pix[(2 * q + 1) * 256 + tid] + ch]) / ((double)w[2 * q + 1] + 1.0);
                col[q] = cc;
            }
        }
    }
#pragma unroll
    for (int z = 0; z < TSDF_R; z++)
        if ((upd >> z) & 1u) {
            f[z] = (f[z] * w[z] + s_tv[z * 256 + tid]) / (w[z] + 1.0f);
            w[z] = w[z] + 1.0f;
        }
#pragma unroll
    for (int q = 0; q < 4; q++) {
        if (!((upd >> (4 * q)) & 15u)) continue;
        reinterpret_cast<float4 *>(tsdf + base)[q] = make_float4(f[q * 4], f[q * 4 + 1], f[q * 4 + 2], f[q * 4 + 3]);
        reinterpret_cast<float4 *>(weight + base)[q] = make_float4(w[q * 4], w[q * 4 + 1], w[q * 4 + 2], w[q * 4 + 3]);
    }
}

// ---- key order --------------------------------------------------------------------------------------------------------------------
// order[r] = the slot whose key has r smaller keys: keys are distinct, so this is a permutation.  n^2 / 2 comparisons out of LDS,
// no host read; a volume has thousands of units, not millions.
__global__ void __launch_bounds__(256) k_tsdf_rank(const unsigned long long *__restrict__ unit_keys, int n, int *__restrict__ order) {
    __shared__ unsigned long long tile[256];
    const int i = blockIdx.x * 256 + threadIdx.x;
    const unsigned long long mine = i < n ? unit_keys[i] : 0ull;
    int r = 0;
    for (int base = 0; base < n; base += 256) {
        tile[threadIdx.x] = base + (int)threadIdx.x < n ? unit_keys[base + threadIdx.x] : TSDF_EMPTY;
        __syncthreads();
#pragma unroll 8
        for (int j = 0; j < 256; j++) r += tile[j] < mine;
        __syncthreads();
    }
    if (i < n) order[r] = i;
}

// ---- extraction -------------------------------------------------------------------------------------------------------------------
struct TsdfVol {
    TsdfTable t;
    const float *tsdf, *weight;
    const double *c[3];
    double vl, ul;
};

__device__ __forceinline__ bool tsdf_usable(float w, float f) { return w != 0.0f && f < 0.98f && f >= -0.98f; }

// QUIRK_TSDF_NORMAL_IGNORES_WEIGHT: the trilinear value reads tsdf alone (a never-observed voxel counts as 0.0), an absent unit
// is 0.0 throughout
__device__ double tsdf_at(const TsdfVol &V, const double *q) {
    const double half = 0.5 * V.vl;
    int U[3], i0[3];
    double r[3];
    for (int k = 0; k < 3; k++) {
        const double ql = q[k] - half;
        const double u = floor(ql / V.ul);
        if (!(u >= (double)-TSDF_IDX_LIMIT && u < (double)TSDF_IDX_LIMIT)) return 0.0;
        U[k] = (int)u;
        const double g = (ql - u * V.ul) / V.vl;
        int c = (int)floor(g);
        c = c < 0 ? 0 : (c > TSDF_R - 1 ? TSDF_R - 1 : c);
        i0[k] = c;
        r[k] = g - (double)c;
    }
    const int home = tsdf_find(V.t, U[0], U[1], U[2]);
    if (home < 0) return 0.0;
    double f[8];
#pragma unroll
    for (int c = 0; c < 8; c++) {   // corner c sits at i0 + {(0,0,0),(1,0,0),(1,1,0),(0,1,0),(0,0,1),(1,0,1),(1,1,1),(0,1,1)}[c]
        const int off[3] = {((c + 1) >> 1) & 1, (c >> 1) & 1, c >> 2};
        int v[3], W[3];
        bool wrap = false;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            v[k] = i0[k] + off[k];
            W[k] = U[k];
            if (v[k] > TSDF_R - 1) { v[k] = 0; W[k]++; wrap = true; }
        }
        const int slot = wrap ? tsdf_find(V.t, W[0], W[1], W[2]) : home;
        f[c] = slot < 0 ? 0.0 : (double)V.tsdf[(size_t)slot * TSDF_UNIT + (v[0] * TSDF_R + v[1]) * TSDF_R + v[2]];
    }
    const double a = 1.0 - r[0], b = 1.0 - r[1], g = 1.0 - r[2];
    return a * (b * (g * f[0] + r[2] * f[4]) + r[1] * (g * f[3] + r[2] * f[7])) +
           r[0] * (b * (g * f[1] + r[2] * f[5]) + r[1] * (g * f[2] + r[2] * f[6]));
}

// One workgroup per unit in key order, one thread per (x, y) column: its 16 voxels are 16 consecutive flat indices, so walking
// threads in order, z in order, axes in order is the contract's order.  EMIT = false counts (thread offsets inside the unit and
// the unit's total), EMIT = true writes the rows at unit_off[unit] + thread_off.
template <bool EMIT, bool COLOR>
__global__ void __launch_bounds__(256) k_tsdf_extract(TsdfVol V, const int *__restrict__ order, const unsigned long long *__restrict__ unit_keys,
                                                      int *__restrict__ thread_off, int *__restrict__ unit_cnt,
                                                      const long long *__restrict__ unit_off, double *__restrict__ xyz,
                                                      double *__restrict__ nrm, double *__restrict__ col) {
    __shared__ int scan[256];
    const int unit = blockIdx.x, tid = (int)threadIdx.x;
    const int slot = order[unit];
    int X, Y, Z;
    tsdf_unpack(unit_keys[slot], X, Y, Z);
    const int x = tid >> 4, y = tid & 15;
    const int sx = x == TSDF_R - 1 ? tsdf_find(V.t, X + 1, Y, Z) : slot;
    const int sy = y == TSDF_R - 1 ? tsdf_find(V.t, X, Y + 1, Z) : slot;
    const int sz = tsdf_find(V.t, X, Y, Z + 1);
    const long long own = (long long)slot * TSDF_UNIT + tid * TSDF_R;
    const long long nbx = sx < 0 ? -1 : (long long)sx * TSDF_UNIT + ((((x + 1) & 15) * TSDF_R) + y) * TSDF_R;
    const long long nby = sy < 0 ? -1 : (long long)sy * TSDF_UNIT + ((x * TSDF_R) + ((y + 1) & 15)) * TSDF_R;
    const long long nbz = sz < 0 ? -1 : (long long)sz * TSDF_UNIT + tid * TSDF_R;
    long long out = 0;
    if (EMIT) out = unit_off[unit] + thread_off[(size_t)unit * 256 + tid];
    int n = 0;
    const double half = 0.5 * V.vl;
    for (int z = 0; z < TSDF_R; z++) {
        const float f0 = V.tsdf[own + z], w0 = V.weight[own + z];
        if (!tsdf_usable(w0, f0)) continue;
        for (int a = 0; a < 3; a++) {
            long long nb;
            if (a == 0) nb = nbx < 0 ? -1 : nbx + z;
            else if (a == 1) nb = nby < 0 ? -1 : nby + z;
            else nb = z < TSDF_R - 1 ? own + z + 1 : nbz;
            if (nb < 0) continue;
            const float f1 = V.tsdf[nb], w1 = V.weight[nb];
            if (!(tsdf_usable(w1, f1) && f0 * f1 < 0.0f)) continue;
            if (EMIT) {
                const float r0f = fabsf(f0), r1f = fabsf(f1);
                const double r0 = (double)r0f, r1 = (double)r1f, rs = (double)(r0f + r1f);
                double p[3] = {(half + V.vl * (double)x) + (double)X * V.ul, (half + V.vl * (double)y) + (double)Y * V.ul,
                               (half + V.vl * (double)z) + (double)Z * V.ul};
                p[a] = (p[a] * r1 + (p[a] + V.vl) * r0) / rs;
                double *o = xyz + (out + n) * 3;
                o[0] = p[0]; o[1] = p[1]; o[2] = p[2];
                if (COLOR) {
                    double *oc = col + (out + n) * 3;
                    for (int ch = 0; ch < 3; ch++) oc[ch] = ((V.c[ch][own + z] * r1 + V.c[ch][nb] * r0) / rs) / 255.0;
                }
                const double d = 0.99 * V.vl;
                double g[3];
                for (int k = 0; k < 3; k++) {
                    double q[3] = {p[0], p[1], p[2]};
                    q[k] = p[k] + d;
                    const double fp = tsdf_at(V, q);
                    q[k] = p[k] - d;
                    g[k] = fp - tsdf_at(V, q);
                }
                const double len = sqrt((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]);
                double *on = nrm + (out + n) * 3;
                for (int k = 0; k < 3; k++) on[k] = len != 0.0 ? g[k] / len : g[k];
            }
            n++;
        }
    }
    if (EMIT) return;
    scan[tid] = n;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
        const int v = tid >= off ? scan[tid - off] : 0;
        __syncthreads();
        scan[tid] += v;
        __syncthreads();
    }
    thread_off[(size_t)unit * 256 + tid] = scan[tid] - n;
    if (tid == 255) unit_cnt[unit] = scan[255];
}

// exclusive offsets of the units and the total, one workgroup: 256 counts at a time with a carry
__global__ void __launch_bounds__(256) k_tsdf_unit_offsets(const int *__restrict__ unit_cnt, int n, long long *__restrict__ unit_off,
                                                           long long *__restrict__ total) {
    __shared__ long long scan[256];
    const int tid = (int)threadIdx.x;
    long long carry = 0;
    for (int base = 0; base < n; base += 256) {
        const long long mine = base + tid < n ? (long long)unit_cnt[base + tid] : 0;
        scan[tid] = mine;
        __syncthreads();
        for (int off = 1; off < 256; off <<= 1) {
            const long long v = tid >= off ? scan[tid - off] : 0;
            __syncthreads();
            scan[tid] += v;
            __syncthreads();
        }
        if (base + tid < n) unit_off[base + tid] = carry + scan[tid] - mine;
        carry += scan[255];
        __syncthreads();
    }
    if (tid == 0) *total = carry;
}

// the debug dump: unit `order[blockIdx.x]`'s planes into row blockIdx.x
__global__ void __launch_bounds__(256) k_tsdf_gather(TsdfVol V, int color, const int *__restrict__ order, const unsigned long long *__restrict__ unit_keys,
                                                     int32_t *__restrict__ idx3, float *__restrict__ o_tsdf, float *__restrict__ o_weight,
                                                     double *__restrict__ o_color) {
    const int unit = blockIdx.x, slot = order[unit];
    if (threadIdx.x == 0) {
        int X, Y, Z;
        tsdf_unpack(unit_keys[slot], X, Y, Z);
        idx3[unit * 3] = X; idx3[unit * 3 + 1] = Y; idx3[unit * 3 + 2] = Z;
    }
    for (int e = threadIdx.x; e < TSDF_UNIT; e += 256) {
        const size_t s = (size_t)slot * TSDF_UNIT + e, d = (size_t)unit * TSDF_UNIT + e;
        o_tsdf[d] = V.tsdf[s];
        o_weight[d] = V.weight[s];
        if (color)
            for (int ch = 0; ch < 3; ch++) o_color[((size_t)unit * 3 + ch) * TSDF_UNIT + e] = V.c[ch][s];
    }
}

// ---- triangle mesh ----------------------------------------------------------------------------------------------------------------
// Marching cubes over the cubes whose base voxel lies in an existing unit ("Triangle mesh").  A vertex is owned
// by (lower voxel of its edge, axis), so it has one home: 3 ids per voxel, no hash map.  Four passes, each one workgroup per unit in
// key order and one thread per (x, y) column, so thread order, z order, axis order is the contract's order:
//   k_tsdf_mc_cubes     the cube byte of every base voxel (the cube index when the cube is active, else 0) into a plane;
//   k_tsdf_mc_vertices  <false> counts the unit's vertices and triangles per thread, <true> writes the vertices and their ids;
//   k_tsdf_mc_triangles writes the triangles from the ids.
// A pass reads what the pass before wrote for the neighbour units (cube bytes of the -x/-y/-z side, ids of the +x/+y/+z side), so
// they are separate launches; inside a launch no workgroup reads what another writes.  Both planes are indexed by pool slot.
__device__ const int8_t d_mc_tri[256][16] = TSDF_MC_TRI_ROWS;
__device__ const uint8_t d_mc_count[256] = TSDF_MC_COUNT_ROWS;

constexpr unsigned long long tsdf_mc_edge_pack() {
    unsigned long long p = 0;
    for (int e = 0; e < 12; e++) p |= (unsigned long long)TSDF_MC_EDGE[e] << (5 * e);
    return p;
}
constexpr unsigned long long TSDF_MC_EDGE_PACK = tsdf_mc_edge_pack();
constexpr int TSDF_LAT = TSDF_R + 1, TSDF_LAT3 = TSDF_LAT * TSDF_LAT * TSDF_LAT;   // a unit and one layer of its neighbours

// nb[(dx + 1) * 9 + (dy + 1) * 3 + (dz + 1)] = the pool slot of unit (X + dx, Y + dy, Z + dz), -1 when absent or outside +-2^20
__device__ __forceinline__ void tsdf_mc_neighbours(const TsdfTable &t, int X, int Y, int Z, int slot, int *nb) {
    const int tid = (int)threadIdx.x;
    if (tid < 27) nb[tid] = tid == 13 ? slot : tsdf_find(t, X + tid / 9 - 1, Y + (tid / 3) % 3 - 1, Z + tid % 3 - 1);
    __syncthreads();
}
// number of the cube corner at offset (ox, oy, oz)
__device__ __forceinline__ int tsdf_mc_corner(int ox, int oy, int oz) { return (oy ? 3 - ox : ox) + 4 * oz; }

__global__ void __launch_bounds__(256) k_tsdf_mc_cubes(TsdfVol V, const int *__restrict__ order, const unsigned long long *__restrict__ unit_keys,
                                                       uint8_t *__restrict__ cube) {
    __shared__ int nb[27];
    __shared__ uint8_t lat[TSDF_LAT3];   // corners 0..16 per axis: bit 0 = its unit exists and its weight is not 0, bit 1 = tsdf < 0
    const int unit = blockIdx.x, tid = (int)threadIdx.x;
    const int slot = order[unit];
    int X, Y, Z;
    tsdf_unpack(unit_keys[slot], X, Y, Z);
    tsdf_mc_neighbours(V.t, X, Y, Z, slot, nb);
    for (int e = tid; e < TSDF_LAT3; e += 256) {
        const int cz = e % TSDF_LAT, cy = (e / TSDF_LAT) % TSDF_LAT, cx = e / (TSDF_LAT * TSDF_LAT);
        const int s = nb[((cx >> 4) + 1) * 9 + ((cy >> 4) + 1) * 3 + (cz >> 4) + 1];
        unsigned f = 0;
        if (s >= 0) {
            const size_t i = (size_t)s * TSDF_UNIT + (((cx & 15) * TSDF_R) + (cy & 15)) * TSDF_R + (cz & 15);
            f = (V.weight[i] != 0.0f ? 1u : 0u) | (V.tsdf[i] < 0.0f ? 2u : 0u);
        }
        lat[e] = (uint8_t)f;
    }
    __syncthreads();
    const int x = tid >> 4, y = tid & 15;
    unsigned w[4] = {0, 0, 0, 0};
#pragma unroll
    for (int z = 0; z < TSDF_R; z++) {
        unsigned all = 1u, index = 0;
#pragma unroll
        for (int c = 0; c < 8; c++) {
            const unsigned f = lat[((x + (((c + 1) >> 1) & 1)) * TSDF_LAT + y + ((c >> 1) & 1)) * TSDF_LAT + z + (c >> 2)];
            all &= f;
            index |= ((f >> 1) & 1u) << c;
        }
        w[z >> 2] |= (all ? index : 0u) << (8 * (z & 3));
    }
    reinterpret_cast<uint4 *>(cube + (size_t)slot * TSDF_UNIT)[tid] = make_uint4(w[0], w[1], w[2], w[3]);
}

// EMIT = false: thread_cnt[unit][thread] = the exclusive sums of (vertices | triangles << 16) over the unit's threads (a unit has at
// most 12288 and 20480), unit_nv / unit_nt the unit's totals.  EMIT = true: the vertex rows at unit_off[unit] + the thread's
// offset, and every voxel's three ids (-1: no vertex) into vid.
template <bool EMIT, bool COLOR>
__global__ void __launch_bounds__(256) k_tsdf_mc_vertices(TsdfVol V, const int *__restrict__ order, const unsigned long long *__restrict__ unit_keys,
                                                          const uint8_t *__restrict__ cube, unsigned *__restrict__ thread_cnt, int *__restrict__ unit_nv,
                                                          int *__restrict__ unit_nt, const long long *__restrict__ unit_off, int32_t *__restrict__ vid,
                                                          double *__restrict__ xyz, double *__restrict__ col) {
    __shared__ int nb[27];
    __shared__ uint8_t cl[TSDF_LAT3];    // cube bytes of the base voxels -1..15 per axis, voxel v at v + 1
    __shared__ unsigned scan[256];
    const int unit = blockIdx.x, tid = (int)threadIdx.x;
    const int slot = order[unit];
    int X, Y, Z;
    tsdf_unpack(unit_keys[slot], X, Y, Z);
    tsdf_mc_neighbours(V.t, X, Y, Z, slot, nb);
    for (int e = tid; e < TSDF_LAT3; e += 256) {
        const int vz = e % TSDF_LAT - 1, vy = (e / TSDF_LAT) % TSDF_LAT - 1, vx = e / (TSDF_LAT * TSDF_LAT) - 1;
        const int s = nb[((vx >> 4) + 1) * 9 + ((vy >> 4) + 1) * 3 + (vz >> 4) + 1];
        cl[e] = s < 0 ? (uint8_t)0 : cube[(size_t)s * TSDF_UNIT + (((vx & 15) * TSDF_R) + (vy & 15)) * TSDF_R + (vz & 15)];
    }
    __syncthreads();
    const int x = tid >> 4, y = tid & 15;
    const long long own = (long long)slot * TSDF_UNIT + tid * TSDF_R;
    long long up[3] = {-1, -1, -1};      // the column of the +1 voxel along x and y, the column above along z
    long long out = 0;
    if (EMIT) {
        const int sx = x == TSDF_R - 1 ? nb[22] : slot, sy = y == TSDF_R - 1 ? nb[16] : slot, sz = nb[14];
        if (sx >= 0) up[0] = (long long)sx * TSDF_UNIT + ((((x + 1) & 15) * TSDF_R) + y) * TSDF_R;
        if (sy >= 0) up[1] = (long long)sy * TSDF_UNIT + ((x * TSDF_R) + ((y + 1) & 15)) * TSDF_R;
        if (sz >= 0) up[2] = (long long)sz * TSDF_UNIT + tid * TSDF_R;
        out = unit_off[unit] + (long long)(thread_cnt[(size_t)unit * 256 + tid] & 0xFFFFu);
    }
    int nv = 0, nt = 0;
    for (int z = 0; z < TSDF_R; z++) {
        const int h[3] = {x + 1, y + 1, z + 1};   // this voxel in cl
        if (!EMIT) nt += d_mc_count[cl[(h[0] * TSDF_LAT + h[1]) * TSDF_LAT + h[2]]];
#pragma unroll
        for (int a = 0; a < 3; a++) {
            // the edge from this voxel along a: a vertex iff one of the four cubes around it is active and has its ends on two sides
            const int b = (a + 1) % 3, c = (a + 2) % 3;
            bool exists = false;
#pragma unroll
            for (int q = 0; q < 4; q++) {
                int d[3] = {0, 0, 0};     // this voxel's offset inside the cube with base voxel h - d
                d[b] = q & 1;
                d[c] = q >> 1;
                const unsigned B = cl[((h[0] - d[0]) * TSDF_LAT + h[1] - d[1]) * TSDF_LAT + h[2] - d[2]];
                const int lo = tsdf_mc_corner(d[0], d[1], d[2]);
                d[a] = 1;
                const int hi = tsdf_mc_corner(d[0], d[1], d[2]);
                exists |= (((B >> lo) ^ (B >> hi)) & 1u) != 0;     // an inactive cube has B = 0
            }
            if (EMIT) {
                int32_t id = -1;
                if (exists) {
                    id = (int32_t)(out + nv);
                    const long long hi = a == 2 ? (z < TSDF_R - 1 ? own + z + 1 : up[2]) : (up[a] < 0 ? -1 : up[a] + z);
                    const double f0 = fabs((double)V.tsdf[own + z]), f1 = hi < 0 ? 0.0 : fabs((double)V.tsdf[hi]);   // hi >= 0: an active cube has it
                    const int g[3] = {X * TSDF_R + x, Y * TSDF_R + y, Z * TSDF_R + z};
                    double p[3] = {0.5 * V.vl + V.vl * (double)g[0], 0.5 * V.vl + V.vl * (double)g[1], 0.5 * V.vl + V.vl * (double)g[2]};
                    p[a] += (f0 * V.vl) / (f0 + f1);
                    double *o = xyz + (out + nv) * 3;
                    o[0] = p[0]; o[1] = p[1]; o[2] = p[2];
                    if (COLOR) {
                        double *oc = col + (out + nv) * 3;
                        for (int ch = 0; ch < 3; ch++) {
                            const double c0 = V.c[ch][own + z], c1 = hi < 0 ? 0.0 : V.c[ch][hi];
                            oc[ch] = ((f1 * c0 + f0 * c1) / (f0 + f1)) / 255.0;
                        }
                    }
                }
                vid[(own + z) * 3 + a] = id;
            }
            nv += exists;
        }
    }
    if (EMIT) return;
    const unsigned mine = (unsigned)nv | (unsigned)nt << 16;
    scan[tid] = mine;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
        const unsigned v = tid >= off ? scan[tid - off] : 0;
        __syncthreads();
        scan[tid] += v;
        __syncthreads();
    }
    thread_cnt[(size_t)unit * 256 + tid] = scan[tid] - mine;
    if (tid == 255) {
        unit_nv[unit] = (int)(scan[255] & 0xFFFFu);
        unit_nt[unit] = (int)(scan[255] >> 16);
    }
}

// triangles of the cubes with their base voxel in the unit: vertex ids of the edges (t0, t2, t1) of every table triple (Open3D's
// swap: with "bit set = negative = inside" the faces look outward)
__global__ void __launch_bounds__(256) k_tsdf_mc_triangles(TsdfTable t, const int *__restrict__ order, const unsigned long long *__restrict__ unit_keys,
                                                           const uint8_t *__restrict__ cube, const int32_t *__restrict__ vid,
                                                           const unsigned *__restrict__ thread_cnt, const long long *__restrict__ unit_off,
                                                           int32_t *__restrict__ tri) {
    __shared__ int nb[27];
    const int unit = blockIdx.x, tid = (int)threadIdx.x;
    const int slot = order[unit];
    int X, Y, Z;
    tsdf_unpack(unit_keys[slot], X, Y, Z);
    tsdf_mc_neighbours(t, X, Y, Z, slot, nb);
    const int x = tid >> 4, y = tid & 15;
    const uint4 mine = reinterpret_cast<const uint4 *>(cube + (size_t)slot * TSDF_UNIT)[tid];
    const unsigned w[4] = {mine.x, mine.y, mine.z, mine.w};
    long long out = unit_off[unit] + (long long)(thread_cnt[(size_t)unit * 256 + tid] >> 16);
    for (int z = 0; z < TSDF_R; z++) {
        const unsigned B = (w[z >> 2] >> (8 * (z & 3))) & 0xFFu;
        const int n = d_mc_count[B];
        for (int k = 0; k < n; k++) {
            int32_t id[3];
            for (int j = 0; j < 3; j++) {
                const unsigned code = (unsigned)(TSDF_MC_EDGE_PACK >> (5 * d_mc_tri[B][3 * k + j])) & 31u;
                const int vx = x + (int)(code & 1u), vy = y + (int)((code >> 1) & 1u), vz = z + (int)((code >> 2) & 1u);
                const int s = nb[((vx >> 4) + 1) * 9 + ((vy >> 4) + 1) * 3 + (vz >> 4) + 1];   // an active cube has all its corner units
                id[j] = s < 0 ? -1 : vid[((size_t)s * TSDF_UNIT + (((vx & 15) * TSDF_R) + (vy & 15)) * TSDF_R + (vz & 15)) * 3 + (code >> 3)];
            }
            int32_t *o = tri + out * 3;
            o[0] = id[0]; o[1] = id[2]; o[2] = id[1];
            out++;
        }
    }
}

}  // namespace

// ---- host side ----------------------------------------------------------------------------------------------------------------------
struct r3d_tsdf {
    r3d_ctx *ctx = nullptr;
    r3d_tsdf_params prm = {};
    int cap = 0;                 // pool capacity in units
    int n_units = 0;
    r3d_buf keys, slot, stamp;   // the hash table's arrays, tcap entries each (TsdfTable is the view kernels get)
    int tcap = 0;
    r3d_buf tsdf, weight, c[3];  // planes of cap units
    r3d_buf unit_keys, order;    // cap entries
    r3d_buf new_list, touched;   // tcap entries
    r3d_buf d_cnt;
    r3d_pinned h_cnt;
    int pass = 0;
    long long frames = 0;
    int last_touched = 0, growths = 0;
    r3d_events<3> ev;
    bool timed = false;

    TsdfTable table() const { return TsdfTable{(unsigned long long *)keys.p, (int *)slot.p, (int *)stamp.p, tcap}; }
};

namespace {

int tsdf_clear_table(r3d_tsdf *v) {
    r3d_ctx *ctx = v->ctx;
    R3D_HIP(ctx, hipMemsetAsync(v->keys.p, 0xFF, (size_t)v->tcap * 8, ctx->stream));
    R3D_HIP(ctx, hipMemsetAsync(v->stamp.p, 0, (size_t)v->tcap * 4, ctx->stream));
    R3D_HIP(ctx, hipMemsetAsync(v->slot.p, 0xFF, (size_t)v->tcap * 4, ctx->stream));
    v->pass = 0;
    if (v->n_units)
        k_tsdf_rebuild<<<(unsigned)((v->n_units + 255) / 256), 256, 0, ctx->stream>>>(v->table(), (const unsigned long long *)v->unit_keys.p, v->n_units);
    R3D_HIP(ctx, hipGetLastError());
    return R3D_OK;
}

// pool of new_cap units and a table of at least twice as many entries; the units kept, the table rebuilt from them.  Commits on
// success: each plane is replaced only once its successor is allocated, copied and zeroed (a plane longer than the pool is
// harmless), and the arrays that hold nothing worth keeping are built aside and moved in together with the capacities.  A failure
// leaves the old capacity, the old arrays and a table the caller rebuilds with tsdf_clear_table.
int tsdf_resize(r3d_tsdf *v, int new_cap) {
    r3d_ctx *ctx = v->ctx;
    hipStream_t st = ctx->stream;
    int rc;
    // a plane of new_cap units from one of v->cap: the first n_units blocks copied, the rest zero
    auto grow_plane = [&](r3d_buf &b, size_t unit_bytes) {
        return b.reserve(ctx, st, (size_t)new_cap * unit_bytes, R3D_GROW_TSDF, (size_t)v->n_units * unit_bytes, true);
    };
    if ((rc = grow_plane(v->tsdf, TSDF_UNIT * 4)) || (rc = grow_plane(v->weight, TSDF_UNIT * 4))) return rc;
    if (v->prm.color_type == R3D_TSDF_COLOR_RGB8)
        for (auto &p : v->c)
            if ((rc = grow_plane(p, TSDF_UNIT * 8))) return rc;
    if ((rc = grow_plane(v->unit_keys, 8))) return rc;
    int tcap = 16;
    while (tcap < 2 * new_cap) tcap *= 2;
    r3d_buf order, keys, slot, stamp, new_list, touched;
    if ((rc = order.reserve(ctx, st, (size_t)new_cap * 4, R3D_GROW_TSDF)) || (rc = keys.reserve(ctx, st, (size_t)tcap * 8, R3D_GROW_TSDF)) ||
        (rc = slot.reserve(ctx, st, (size_t)tcap * 4, R3D_GROW_TSDF)) || (rc = stamp.reserve(ctx, st, (size_t)tcap * 4, R3D_GROW_TSDF)) ||
        (rc = new_list.reserve(ctx, st, (size_t)tcap * 4, R3D_GROW_TSDF)) || (rc = touched.reserve(ctx, st, (size_t)tcap * 4, R3D_GROW_TSDF)))
        return rc;
    v->order = std::move(order);
    v->keys = std::move(keys); v->slot = std::move(slot); v->stamp = std::move(stamp);
    v->new_list = std::move(new_list); v->touched = std::move(touched);
    v->tcap = tcap;
    v->cap = new_cap;
    return tsdf_clear_table(v);
}

int tsdf_vol_ok(r3d_ctx *ctx, const r3d_tsdf *v, const char *who) {
    if (!v) return r3d_fail(ctx, R3D_E_BADARG, "%s: volume missing", who);
    if (v->ctx != ctx) return r3d_fail(ctx, R3D_E_BADARG, "%s: the volume belongs to another context", who);
    if (ctx->poisoned) return r3d_fail(ctx, R3D_E_HIP, "%s: context poisoned by an earlier timed-out call: destroy it", who);
    return R3D_OK;
}

// inverse of an affine 4x4 by the adjugate of its 3x3 block, every expression in the order tests/tsdf_ref.py writes it
int tsdf_inverse(r3d_ctx *ctx, const double *E, TsdfPose &P) {
    if (!(E[12] == 0.0 && E[13] == 0.0 && E[14] == 0.0 && E[15] == 1.0))
        return r3d_fail(ctx, R3D_E_BADARG, "tsdf_integrate: the extrinsic's last row must be 0 0 0 1");
    const double a = E[0], b = E[1], c = E[2], d = E[4], e = E[5], f = E[6], g = E[8], h = E[9], i = E[10];
    const double det = (a * (e * i - f * h) + b * (f * g - d * i)) + c * (d * h - e * g);
    if (!std::isfinite(det) || det == 0.0) return r3d_fail(ctx, R3D_E_BADARG, "tsdf_integrate: the extrinsic is singular or not finite");
    const double adj[9] = {e * i - f * h, c * h - b * i, b * f - c * e, f * g - d * i, a * i - c * g, c * d - a * f, d * h - e * g, b * g - a * h, a * e - b * d};
    for (int k = 0; k < 9; k++) P.Ai[k] = adj[k] / det;
    for (int k = 0; k < 3; k++) P.ti[k] = -((P.Ai[k * 3] * E[3] + P.Ai[k * 3 + 1] * E[7]) + P.Ai[k * 3 + 2] * E[11]);
    for (int k = 0; k < 3; k++)
        if (!std::isfinite(P.ti[k])) return r3d_fail(ctx, R3D_E_BADARG, "tsdf_integrate: the extrinsic is singular or not finite");
    return R3D_OK;
}

int tsdf_images_ok(r3d_ctx *ctx, const r3d_tsdf *v, const void *depth, const void *color, int w, int h, int dstride, int cw, int ch, int cstride, int cn,
                   double fx, double fy, const double *extrinsic) {
    if (!depth || !extrinsic || w <= 0 || h <= 0 || dstride < w || (int64_t)w * h > (int64_t)1 << 28)
        return r3d_fail(ctx, R3D_E_BADARG, "tsdf_integrate: a missing depth image or extrinsic, an empty image or a stride too small");
    if (!(fx != 0) || !(fy != 0) || !std::isfinite(fx) || !std::isfinite(fy)) return r3d_fail(ctx, R3D_E_BADARG, "tsdf_integrate: fx and fy must be non-zero");
    if (v->prm.color_type == R3D_TSDF_COLOR_RGB8) {
        if (!color || cn != 3) return r3d_fail(ctx, R3D_E_BADARG, "tsdf_integrate: an RGB8 volume needs a 3-channel colour image (got %d channels)", color ? cn : 0);
        if (cw != w || ch != h) return r3d_fail(ctx, R3D_E_BADARG, "tsdf_integrate: colour image %d x %d and depth image %d x %d differ in size", cw, ch, w, h);
        if ((int64_t)cstride < (int64_t)w * 3 || (int64_t)cstride * h > INT32_MAX) return r3d_fail(ctx, R3D_E_BADARG, "tsdf_integrate: colour stride %d", cstride);
    }
    return R3D_OK;
}

// device planes in; everything up to and including the integrate launch
int tsdf_integrate_dev(r3d_tsdf *v, const float *d_depth, int dstride, const uint8_t *d_color, int cstride, int w, int h, TsdfCam cam, const double *E) {
    r3d_ctx *ctx = v->ctx;
    hipStream_t st = ctx->stream;
    TsdfPose P;
    if (int rc = tsdf_inverse(ctx, E, P)) return rc;
    const int s = v->prm.depth_sampling_stride;
    const int ni = (h + s - 1) / s, nj = (w + s - 1) / s;
    const double ul = v->prm.voxel_length * TSDF_R;
    R3D_HIP(ctx, hipEventRecord(v->ev[0], st));
    TsdfCounters cnt;
    for (;;) {
        v->pass++;
        R3D_HIP(ctx, hipMemsetAsync(v->d_cnt.p, 0, sizeof(TsdfCounters), st));
        k_tsdf_touch<<<(unsigned)(((size_t)ni * nj + 255) / 256), 256, 0, st>>>(d_depth, dstride, s, nj, ni, cam, P, v->prm.sdf_trunc, ul, v->table(), v->pass,
                                                                                 (int *)v->new_list.p, (int *)v->touched.p, (TsdfCounters *)v->d_cnt.p);
        R3D_HIP(ctx, hipGetLastError());
        // the one device -> host read of a frame: 16 bytes of counters (a frame that outgrows the pool repeats the pass and the read)
        R3D_HIP(ctx, hipMemcpyAsync(v->h_cnt.p, v->d_cnt.p, sizeof(TsdfCounters), hipMemcpyDeviceToHost, st));
        R3D_HIP(ctx, hipStreamSynchronize(st));
        cnt = *(const TsdfCounters *)v->h_cnt.p;
        if (cnt.out_of_range) {
            if (int rc = tsdf_clear_table(v)) return rc;
            return r3d_fail(ctx, R3D_E_UNSUPPORTED, "tsdf_integrate: a depth sample falls into a unit index outside +-2^20 (or is not finite)");
        }
        if (!cnt.table_full && v->n_units + cnt.n_new <= v->cap) break;
        int want = v->n_units + cnt.n_new;
        if (want < 2 * v->cap) want = 2 * v->cap;
        if (want > (1 << 22)) {
            (void)tsdf_clear_table(v);
            return r3d_fail(ctx, R3D_E_OOM, "tsdf_integrate: more than 2^22 units");
        }
        if (int rc = tsdf_resize(v, want)) {
            // the touch pass has put keys without slots into the table: rebuild it from the units, keep the allocation's message
            const std::string why = ctx->err;
            (void)tsdf_clear_table(v);
            ctx->err = why;
            return rc;
        }
        v->growths++;
    }
    if (cnt.n_new) k_tsdf_assign<<<(unsigned)((cnt.n_new + 255) / 256), 256, 0, st>>>(v->table(), (const int *)v->new_list.p, cnt.n_new, v->n_units, (unsigned long long *)v->unit_keys.p);
    v->n_units += cnt.n_new;
    R3D_HIP(ctx, hipEventRecord(v->ev[1], st));
    if (cnt.n_touched) {
        TsdfFrame F;
        F.depth = d_depth; F.color = d_color; F.dstride = dstride; F.cstride = cstride; F.w = w; F.h = h;
        F.fx = (float)cam.fx; F.fy = (float)cam.fy; F.cx = (float)cam.cx; F.cy = (float)cam.cy;
        F.ifx = 1.0f / F.fx; F.ify = 1.0f / F.fy;
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 4; c++) F.E[r * 4 + c] = (float)E[r * 4 + c];
        F.vl = (float)v->prm.voxel_length; F.trunc = (float)v->prm.sdf_trunc; F.itrunc = 1.0f / F.trunc;
        F.wlim = (float)((double)w - 0.0001); F.hlim = (float)((double)h - 0.0001);
        F.vld = v->prm.voxel_length; F.ul = ul;
        if (v->prm.color_type == R3D_TSDF_COLOR_RGB8)
            k_tsdf_integrate<true><<<(unsigned)cnt.n_touched, 256, 0, st>>>(F, v->table(), (const int *)v->touched.p, (float *)v->tsdf.p, (float *)v->weight.p, (double *)v->c[0].p, (double *)v->c[1].p, (double *)v->c[2].p);
        else
            k_tsdf_integrate<false><<<(unsigned)cnt.n_touched, 256, 0, st>>>(F, v->table(), (const int *)v->touched.p, (float *)v->tsdf.p, (float *)v->weight.p, nullptr, nullptr, nullptr);
        R3D_HIP(ctx, hipGetLastError());
    }
    R3D_HIP(ctx, hipEventRecord(v->ev[2], st));
    v->timed = true;
    v->frames++;
    v->last_touched = cnt.n_touched;
    return R3D_OK;
}

TsdfVol tsdf_view(const r3d_tsdf *v) {
    TsdfVol V;
    V.t = v->table(); V.tsdf = (const float *)v->tsdf.p; V.weight = (const float *)v->weight.p;
    for (int k = 0; k < 3; k++) V.c[k] = (const double *)v->c[k].p;
    V.vl = v->prm.voxel_length; V.ul = v->prm.voxel_length * TSDF_R;
    return V;
}

int tsdf_sort_units(r3d_tsdf *v) {
    if (v->n_units) k_tsdf_rank<<<(unsigned)((v->n_units + 255) / 256), 256, 0, v->ctx->stream>>>((const unsigned long long *)v->unit_keys.p, v->n_units, (int *)v->order.p);
    R3D_HIP(v->ctx, hipGetLastError());
    return R3D_OK;
}

// extraction in two halves around the caller's capacity check: the count (always), then the rows into device arrays
struct TsdfExtractWork {
    int n = 0;   // units
    int *thread_off = nullptr, *unit_cnt = nullptr;
    long long *unit_off = nullptr, total = 0;
};
// allocates the scratch, counts, and returns after its one synchronisation with the total in W and *out_n (0 for an empty volume)
int tsdf_extract_count(r3d_tsdf *v, DevArena &ar, TsdfExtractWork &W, int64_t *out_n) {
    r3d_ctx *ctx = v->ctx;
    hipStream_t st = ctx->stream;
    *out_n = 0;
    if (!v->n_units) return R3D_OK;
    const int n = W.n = v->n_units;
    W.thread_off = (int *)ar.get((size_t)n * 256 * 4);
    W.unit_cnt = (int *)ar.get((size_t)n * 4);
    W.unit_off = (long long *)ar.get((size_t)n * 8);
    long long *d_total = (long long *)ar.get(8);
    if (ar.rc) return ar.rc;
    if (int rc = tsdf_sort_units(v)) return rc;
    k_tsdf_extract<false, false><<<(unsigned)n, 256, 0, st>>>(tsdf_view(v), (const int *)v->order.p, (const unsigned long long *)v->unit_keys.p, W.thread_off, W.unit_cnt, nullptr, nullptr, nullptr, nullptr);
    k_tsdf_unit_offsets<<<1, 256, 0, st>>>(W.unit_cnt, n, W.unit_off, d_total);
    R3D_HIP(ctx, hipGetLastError());
    if (int rc = r3d_read_back(ctx, {{&W.total, d_total, 8}})) return rc;
    *out_n = W.total;
    return R3D_OK;
}
// W.total > 0 rows into device arrays (d_col only for a coloured volume); enqueues only
int tsdf_extract_emit(r3d_tsdf *v, const TsdfExtractWork &W, double *d_xyz, double *d_nrm, double *d_col) {
    if (v->prm.color_type == R3D_TSDF_COLOR_RGB8)
        k_tsdf_extract<true, true><<<(unsigned)W.n, 256, 0, v->ctx->stream>>>(tsdf_view(v), (const int *)v->order.p, (const unsigned long long *)v->unit_keys.p, W.thread_off, W.unit_cnt, W.unit_off, d_xyz, d_nrm, d_col);
    else
        k_tsdf_extract<true, false><<<(unsigned)W.n, 256, 0, v->ctx->stream>>>(tsdf_view(v), (const int *)v->order.p, (const unsigned long long *)v->unit_keys.p, W.thread_off, W.unit_cnt, W.unit_off, d_xyz, d_nrm, nullptr);
    R3D_HIP(v->ctx, hipGetLastError());
    return R3D_OK;
}

// the mesh likewise: cube bytes and counts (always), then vertices, ids and triangles into device arrays
struct TsdfMeshWork {
    int n = 0;   // units
    TsdfVol V;
    const int *order = nullptr;               // v->order and v->unit_keys, typed
    const unsigned long long *keys = nullptr;
    uint8_t *cube = nullptr;
    unsigned *thread_cnt = nullptr;
    int32_t *vid = nullptr;   // the emitting half's vertex ids (tsdf_mesh_fits)
    long long *unit_off = nullptr, total[2] = {0, 0};   // total: vertices, triangles
};
// as tsdf_extract_count, with the totals in W, *out_nv and *out_nt; refuses totals that int32 triangle indices cannot address
int tsdf_mesh_count(r3d_tsdf *v, DevArena &ar, TsdfMeshWork &W, int64_t *out_nv, int64_t *out_nt) {
    r3d_ctx *ctx = v->ctx;
    hipStream_t st = ctx->stream;
    *out_nv = *out_nt = 0;
    if (!v->n_units) return R3D_OK;
    const int n = W.n = v->n_units;
    W.cube = (uint8_t *)ar.get((size_t)n * TSDF_UNIT);
    W.thread_cnt = (unsigned *)ar.get((size_t)n * 256 * 4);
    int *unit_cnt = (int *)ar.get((size_t)n * 2 * 4);              // vertices of every unit, then triangles of every unit
    W.unit_off = (long long *)ar.get((size_t)n * 2 * 8);
    long long *d_total = (long long *)ar.get(16);
    if (ar.rc) return ar.rc;
    if (int rc = tsdf_sort_units(v)) return rc;
    W.V = tsdf_view(v);
    W.order = (const int *)v->order.p;
    W.keys = (const unsigned long long *)v->unit_keys.p;
    k_tsdf_mc_cubes<<<(unsigned)n, 256, 0, st>>>(W.V, W.order, W.keys, W.cube);
    k_tsdf_mc_vertices<false, false><<<(unsigned)n, 256, 0, st>>>(W.V, W.order, W.keys, W.cube, W.thread_cnt, unit_cnt, unit_cnt + n, nullptr, nullptr, nullptr, nullptr);
    k_tsdf_unit_offsets<<<1, 256, 0, st>>>(unit_cnt, n, W.unit_off, d_total);
    k_tsdf_unit_offsets<<<1, 256, 0, st>>>(unit_cnt + n, n, W.unit_off + n, d_total + 1);
    R3D_HIP(ctx, hipGetLastError());
    if (int rc = r3d_read_back(ctx, {{W.total, d_total, 16}})) return rc;
    *out_nv = W.total[0]; *out_nt = W.total[1];
    if (W.total[0] > INT32_MAX || W.total[1] > INT32_MAX)
        return r3d_fail(ctx, R3D_E_UNSUPPORTED, "mesh_from_volume: %lld vertices and %lld triangles do not fit int32 indices", W.total[0], W.total[1]);
    return R3D_OK;
}
// the capacity refusal of a non-empty mesh, then the emitting half's scratch: it comes ahead of any arena outputs of the caller
int tsdf_mesh_fits(r3d_ctx *ctx, DevArena &ar, TsdfMeshWork &W, int64_t cap_v, int64_t cap_t) {
    if (int rc = r3d_fits2(ctx, "mesh_from_volume", "vertices", W.total[0], "triangles", W.total[1], cap_v, cap_t)) return rc;
    W.vid = (int32_t *)ar.get((size_t)W.n * TSDF_UNIT * 12);
    return ar.rc;
}
// the counted mesh into device arrays (d_col only for a coloured volume); enqueues only
int tsdf_mesh_emit(r3d_tsdf *v, const TsdfMeshWork &W, double *d_vert, double *d_col, int32_t *d_tri) {
    hipStream_t st = v->ctx->stream;
    if (v->prm.color_type == R3D_TSDF_COLOR_RGB8)
        k_tsdf_mc_vertices<true, true><<<(unsigned)W.n, 256, 0, st>>>(W.V, W.order, W.keys, W.cube, W.thread_cnt, nullptr, nullptr, W.unit_off, W.vid, d_vert, d_col);
    else
        k_tsdf_mc_vertices<true, false><<<(unsigned)W.n, 256, 0, st>>>(W.V, W.order, W.keys, W.cube, W.thread_cnt, nullptr, nullptr, W.unit_off, W.vid, d_vert, nullptr);
    k_tsdf_mc_triangles<<<(unsigned)W.n, 256, 0, st>>>(W.V.t, W.order, W.keys, W.cube, W.vid, W.thread_cnt, W.unit_off + W.n, d_tri);
    R3D_HIP(v->ctx, hipGetLastError());
    return R3D_OK;
}

int tsdf_mesh_args_ok(r3d_ctx *ctx, const r3d_tsdf *v, int64_t cap_v, int64_t cap_t, const void *vert, const void *col, const void *tri, const void *out_nv,
                      const void *out_nt) {
    if (int rc = tsdf_vol_ok(ctx, v, "mesh_from_volume")) return rc;
    const bool color = v->prm.color_type == R3D_TSDF_COLOR_RGB8;
    if (!out_nv || !out_nt || cap_v < 0 || cap_t < 0 || (cap_v > 0 && (!vert || (color && !col))) || (cap_t > 0 && !tri))
        return r3d_fail(ctx, R3D_E_BADARG, "mesh_from_volume: a missing array or a negative capacity");
    return R3D_OK;
}

}  // namespace

extern "C" {

int r3d_tsdf_create(r3d_ctx *ctx, const r3d_tsdf_params *p, r3d_tsdf **out) {
    R3D_ROCTX_RANGE("r3d_tsdf_create");
    if (!ctx) return R3D_E_BADARG;
    if (!p || !out) return r3d_fail(ctx, R3D_E_BADARG, "tsdf_create: params or output missing");
    *out = nullptr;
    if (!(p->voxel_length > 0) || !std::isfinite(p->voxel_length)) return r3d_fail(ctx, R3D_E_BADARG, "tsdf_create: voxel_length must be positive");
    if (!(p->sdf_trunc > 0) || !std::isfinite(p->sdf_trunc)) return r3d_fail(ctx, R3D_E_BADARG, "tsdf_create: sdf_trunc must be positive");
    if (p->depth_sampling_stride < 1) return r3d_fail(ctx, R3D_E_BADARG, "tsdf_create: depth_sampling_stride %d < 1", p->depth_sampling_stride);
    if (p->color_type != R3D_TSDF_COLOR_NONE && p->color_type != R3D_TSDF_COLOR_RGB8)
        return r3d_fail(ctx, p->color_type == 2 ? R3D_E_UNSUPPORTED : R3D_E_BADARG, "tsdf_create: color_type %d (0 None, 1 RGB8; Gray32 is not built)", p->color_type);
    if (p->initial_units < 0 || p->initial_units > (1 << 22)) return r3d_fail(ctx, R3D_E_BADARG, "tsdf_create: initial_units %d", p->initial_units);
    if (p->volume_unit_resolution != TSDF_R)
        return r3d_fail(ctx, R3D_E_UNSUPPORTED, "tsdf_create: volume_unit_resolution %d (only 16 is built)", p->volume_unit_resolution);
    if (ctx->poisoned) return r3d_fail(ctx, R3D_E_HIP, "tsdf_create: context poisoned by an earlier timed-out call: destroy it");
    R3D_HIP(ctx, hipSetDevice(ctx->device));
    r3d_tsdf *v = new r3d_tsdf;
    v->ctx = ctx;
    v->prm = *p;
    int rc = v->d_cnt.reserve(ctx, ctx->stream, sizeof(TsdfCounters), R3D_GROW_TSDF);
    if (!rc && v->h_cnt.alloc(sizeof(TsdfCounters), hipHostMallocDefault) != hipSuccess)
        rc = r3d_fail(ctx, R3D_E_OOM, "tsdf_create: pinned allocation failed");
    if (!rc && v->ev.create_all() != hipSuccess) rc = r3d_fail(ctx, R3D_E_HIP, "tsdf_create: hipEventCreate failed");
    if (!rc) rc = tsdf_resize(v, p->initial_units ? p->initial_units : TSDF_DEFAULT_UNITS);
    if (rc) {
        delete v;
        return rc;
    }
    *out = v;
    return R3D_OK;
}

int r3d_tsdf_destroy(r3d_ctx *ctx, r3d_tsdf *vol) {
    R3D_ROCTX_RANGE("r3d_tsdf_destroy");
    if (!ctx) return R3D_E_BADARG;
    if (!vol) return r3d_fail(ctx, R3D_E_BADARG, "tsdf_destroy: volume missing");
    if (vol->ctx != ctx) return r3d_fail(ctx, R3D_E_BADARG, "tsdf_destroy: the volume belongs to another context");
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    delete vol;
    return R3D_OK;
}

int r3d_tsdf_reset(r3d_ctx *ctx, r3d_tsdf *vol) {
    R3D_ROCTX_RANGE("r3d_tsdf_reset");
    if (!ctx) return R3D_E_BADARG;
    if (int rc = tsdf_vol_ok(ctx, vol, "tsdf_reset")) return rc;
    R3D_HIP(ctx, hipSetDevice(ctx->device));
    const size_t used = (size_t)vol->n_units * TSDF_UNIT;
    if (used) {
        R3D_HIP(ctx, hipMemsetAsync(vol->tsdf.p, 0, used * 4, ctx->stream));
        R3D_HIP(ctx, hipMemsetAsync(vol->weight.p, 0, used * 4, ctx->stream));
        if (vol->prm.color_type == R3D_TSDF_COLOR_RGB8)
            for (auto &p : vol->c) R3D_HIP(ctx, hipMemsetAsync(p.p, 0, used * 8, ctx->stream));
    }
    vol->n_units = 0;
    vol->frames = 0;
    vol->last_touched = 0;
    vol->timed = false;
    return tsdf_clear_table(vol);
}

int r3d_tsdf_integrate_f32_dev(r3d_ctx *ctx, r3d_tsdf *vol, const float *d_depth, const uint8_t *d_color, int32_t w, int32_t h, int32_t depth_stride,
                               int32_t color_w, int32_t color_h, int32_t color_stride, int32_t color_channels, double fx, double fy, double cx,
                               double cy, const double *extrinsic4x4) {
    R3D_ROCTX_RANGE("r3d_tsdf_integrate_f32_dev");
    if (!ctx) return R3D_E_BADARG;
    int rc;
    if ((rc = tsdf_vol_ok(ctx, vol, "tsdf_integrate"))) return rc;
    if ((rc = tsdf_images_ok(ctx, vol, d_depth, d_color, w, h, depth_stride, color_w, color_h, color_stride, color_channels, fx, fy, extrinsic4x4))) return rc;
    R3D_HIP(ctx, hipSetDevice(ctx->device));
    return tsdf_integrate_dev(vol, d_depth, depth_stride, d_color, color_stride, w, h, TsdfCam{fx, fy, cx, cy}, extrinsic4x4);
}

int r3d_tsdf_integrate_f32(r3d_ctx *ctx, r3d_tsdf *vol, const float *depth, const uint8_t *color, int32_t w, int32_t h, int32_t depth_stride,
                           int32_t color_w, int32_t color_h, int32_t color_stride, int32_t color_channels, double fx, double fy, double cx, double cy,
                           const double *extrinsic4x4) {
    R3D_ROCTX_RANGE("r3d_tsdf_integrate_f32");
    if (!ctx) return R3D_E_BADARG;
    int rc;
    if ((rc = tsdf_vol_ok(ctx, vol, "tsdf_integrate"))) return rc;
    if ((rc = tsdf_images_ok(ctx, vol, depth, color, w, h, depth_stride, color_w, color_h, color_stride, color_channels, fx, fy, extrinsic4x4))) return rc;
    R3D_HIP(ctx, hipSetDevice(ctx->device));
    const bool rgb = vol->prm.color_type == R3D_TSDF_COLOR_RGB8;
    DevArena ar(ctx);
    float *dd;
    uint8_t *dc = nullptr;
    if ((rc = r3d_upload_plane(ctx, ar, depth, w, h, depth_stride, &dd)) || (rgb && (rc = r3d_upload_plane(ctx, ar, color, w * 3, h, color_stride, &dc)))) return rc;
    if ((rc = tsdf_integrate_dev(vol, dd, w, dc, w * 3, w, h, TsdfCam{fx, fy, cx, cy}, extrinsic4x4))) return rc;
    R3D_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return R3D_OK;
}

int r3d_tsdf_integrate(r3d_ctx *ctx, r3d_tsdf *vol, const uint16_t *depth, const uint8_t *color, int32_t w, int32_t h, int32_t depth_stride,
                       int32_t color_w, int32_t color_h, int32_t color_stride, int32_t color_channels, const r3d_depth_camera *cam,
                       const double *extrinsic4x4) {
    R3D_ROCTX_RANGE("r3d_tsdf_integrate");
    if (!ctx) return R3D_E_BADARG;
    int rc;
    if ((rc = tsdf_vol_ok(ctx, vol, "tsdf_integrate"))) return rc;
    if (!cam) return r3d_fail(ctx, R3D_E_BADARG, "tsdf_integrate: camera missing");
    if (!(cam->depth_scale > 0) || !(cam->depth_trunc > 0)) return r3d_fail(ctx, R3D_E_BADARG, "tsdf_integrate: depth_scale and depth_trunc must be positive");
    if ((rc = tsdf_images_ok(ctx, vol, depth, color, w, h, depth_stride, color_w, color_h, color_stride, color_channels, cam->fx, cam->fy, extrinsic4x4)))
        return rc;
    R3D_HIP(ctx, hipSetDevice(ctx->device));
    const bool rgb = vol->prm.color_type == R3D_TSDF_COLOR_RGB8;
    DevArena ar(ctx);
    uint16_t *raw;
    uint8_t *dc = nullptr;
    if ((rc = r3d_upload_plane(ctx, ar, depth, w, h, depth_stride, &raw))) return rc;
    float *dd = (float *)ar.get((size_t)w * h * 4);
    if (ar.rc) return ar.rc;
    if (rgb && (rc = r3d_upload_plane(ctx, ar, color, w * 3, h, color_stride, &dc))) return rc;
    k_tsdf_depth_u16<<<(unsigned)(((size_t)w * h + 255) / 256), 256, 0, ctx->stream>>>(raw, w, h, (float)cam->depth_scale, (float)cam->depth_trunc, dd);
    R3D_HIP(ctx, hipGetLastError());
    if ((rc = tsdf_integrate_dev(vol, dd, w, dc, w * 3, w, h, TsdfCam{cam->fx, cam->fy, cam->ppx, cam->ppy}, extrinsic4x4))) return rc;
    R3D_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return R3D_OK;
}

int r3d_tsdf_stats(r3d_ctx *ctx, r3d_tsdf *vol, r3d_tsdf_info *out) {
    R3D_ROCTX_RANGE("r3d_tsdf_stats");
    if (!ctx) return R3D_E_BADARG;
    if (int rc = tsdf_vol_ok(ctx, vol, "tsdf_stats")) return rc;
    if (!out) return r3d_fail(ctx, R3D_E_BADARG, "tsdf_stats: output missing");
    memset(out, 0, sizeof(*out));
    out->units = vol->n_units;
    out->frames = vol->frames;
    out->touched = vol->last_touched;
    out->capacity = vol->cap;
    out->growths = vol->growths;
    if (vol->timed) {
        float ms = 0;
        R3D_HIP(ctx, hipEventSynchronize(vol->ev[2]));
        R3D_HIP(ctx, hipEventElapsedTime(&ms, vol->ev[0], vol->ev[1]));
        out->touch_ms = ms;
        R3D_HIP(ctx, hipEventElapsedTime(&ms, vol->ev[1], vol->ev[2]));
        out->integrate_ms = ms;
    }
    return R3D_OK;
}

int r3d_tsdf_extract_point_cloud(r3d_ctx *ctx, r3d_tsdf *vol, int64_t cap, double *xyz, double *normals, double *colors, int64_t *out_n) {
    R3D_ROCTX_RANGE("r3d_tsdf_extract_point_cloud");
    if (!ctx) return R3D_E_BADARG;
    if (int rc = tsdf_vol_ok(ctx, vol, "tsdf_extract_point_cloud")) return rc;
    const bool color = vol->prm.color_type == R3D_TSDF_COLOR_RGB8;
    if (!out_n || cap < 0 || (cap > 0 && (!xyz || !normals || (color && !colors))))
        return r3d_fail(ctx, R3D_E_BADARG, "tsdf_extract_point_cloud: a missing array or a negative capacity");
    R3D_HIP(ctx, hipSetDevice(ctx->device));
    DevArena ar(ctx);
    TsdfExtractWork W;
    int rc;
    if ((rc = tsdf_extract_count(vol, ar, W, out_n))) return rc;
    if (cap == 0 || W.total == 0) return R3D_OK;
    if ((rc = r3d_fits(ctx, "tsdf_extract_point_cloud", "points", W.total, cap))) return rc;
    const size_t n3 = (size_t)W.total * 3;
    double *d_xyz = (double *)ar.get(n3 * 8), *d_nrm = (double *)ar.get(n3 * 8), *d_col = color ? (double *)ar.get(n3 * 8) : nullptr;
    if (ar.rc) return ar.rc;
    if ((rc = tsdf_extract_emit(vol, W, d_xyz, d_nrm, d_col)) || (rc = r3d_download(ctx, xyz, d_xyz, n3)) || (rc = r3d_download(ctx, normals, d_nrm, n3)) ||
        (rc = r3d_download(ctx, colors, d_col, color ? n3 : 0)))
        return rc;
    R3D_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return R3D_OK;
}

int r3d_tsdf_extract_point_cloud_dev(r3d_ctx *ctx, r3d_tsdf *vol, int64_t cap, double *d_xyz, double *d_normals, double *d_colors, int64_t *out_n) {
    R3D_ROCTX_RANGE("r3d_tsdf_extract_point_cloud_dev");
    if (!ctx) return R3D_E_BADARG;
    if (int rc = tsdf_vol_ok(ctx, vol, "tsdf_extract_point_cloud")) return rc;
    const bool color = vol->prm.color_type == R3D_TSDF_COLOR_RGB8;
    if (!out_n || cap < 0 || (cap > 0 && (!d_xyz || !d_normals || (color && !d_colors))))
        return r3d_fail(ctx, R3D_E_BADARG, "tsdf_extract_point_cloud: a missing array or a negative capacity");
    R3D_HIP(ctx, hipSetDevice(ctx->device));
    DevArena ar(ctx);
    TsdfExtractWork W;
    int rc;
    if ((rc = tsdf_extract_count(vol, ar, W, out_n))) return rc;
    if (cap > 0 && W.total > 0 && ((rc = r3d_fits(ctx, "tsdf_extract_point_cloud", "points", W.total, cap)) || (rc = tsdf_extract_emit(vol, W, d_xyz, d_normals, d_colors))))
        return rc;
    R3D_HIP(ctx, hipStreamSynchronize(ctx->stream));   // the emit kernel reads arena buffers the next call may hand out again
    return R3D_OK;
}

int r3d_debug_tsdf_units(r3d_ctx *ctx, r3d_tsdf *vol, int64_t cap_units, int32_t *idx3, float *tsdf, float *weight, double *colour, int64_t *out_n) {
    R3D_ROCTX_RANGE("r3d_debug_tsdf_units");
    if (!ctx) return R3D_E_BADARG;
    if (int rc = tsdf_vol_ok(ctx, vol, "debug_tsdf_units")) return rc;
    const bool color = vol->prm.color_type == R3D_TSDF_COLOR_RGB8;
    if (!out_n || cap_units < 0 || (cap_units > 0 && (!idx3 || !tsdf || !weight || (color && !colour))))
        return r3d_fail(ctx, R3D_E_BADARG, "debug_tsdf_units: a missing array or a negative capacity");
    const int n = vol->n_units;
    *out_n = n;
    if (cap_units == 0 || n == 0) return R3D_OK;
    if (int rc = r3d_fits(ctx, "debug_tsdf_units", "units", n, cap_units)) return rc;
    R3D_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    DevArena ar(ctx);
    int32_t *d_idx = (int32_t *)ar.get((size_t)n * 12);
    float *d_t = (float *)ar.get((size_t)n * TSDF_UNIT * 4), *d_w = (float *)ar.get((size_t)n * TSDF_UNIT * 4);
    double *d_c = color ? (double *)ar.get((size_t)n * TSDF_UNIT * 24) : nullptr;
    if (ar.rc) return ar.rc;
    if (int rc = tsdf_sort_units(vol)) return rc;
    k_tsdf_gather<<<(unsigned)n, 256, 0, st>>>(tsdf_view(vol), color ? 1 : 0, (const int *)vol->order.p, (const unsigned long long *)vol->unit_keys.p, d_idx, d_t, d_w, d_c);
    R3D_HIP(ctx, hipGetLastError());
    const size_t nvox = (size_t)n * TSDF_UNIT;
    int rc;
    if ((rc = r3d_download(ctx, idx3, d_idx, (size_t)n * 3)) || (rc = r3d_download(ctx, tsdf, d_t, nvox)) || (rc = r3d_download(ctx, weight, d_w, nvox)) ||
        (rc = r3d_download(ctx, colour, d_c, color ? nvox * 3 : 0)))
        return rc;
    R3D_HIP(ctx, hipStreamSynchronize(st));
    return R3D_OK;
}

int r3d_mesh_from_volume(r3d_ctx *ctx, r3d_tsdf *vol, int64_t cap_vertices, int64_t cap_triangles, double *vertices, double *colors, int32_t *triangles,
                         int64_t *out_nv, int64_t *out_nt) {
    R3D_ROCTX_RANGE("r3d_mesh_from_volume");
    if (!ctx) return R3D_E_BADARG;
    if (int rc = tsdf_mesh_args_ok(ctx, vol, cap_vertices, cap_triangles, vertices, colors, triangles, out_nv, out_nt)) return rc;
    R3D_HIP(ctx, hipSetDevice(ctx->device));
    DevArena ar(ctx);
    TsdfMeshWork W;
    int rc;
    if ((rc = tsdf_mesh_count(vol, ar, W, out_nv, out_nt))) return rc;
    if ((cap_vertices == 0 && cap_triangles == 0) || (W.total[0] == 0 && W.total[1] == 0)) return R3D_OK;
    if ((rc = tsdf_mesh_fits(ctx, ar, W, cap_vertices, cap_triangles))) return rc;
    const bool color = vol->prm.color_type == R3D_TSDF_COLOR_RGB8;
    const size_t nv3 = (size_t)W.total[0] * 3, nt3 = (size_t)W.total[1] * 3;
    double *d_vert = (double *)ar.get(nv3 * 8), *d_col = color ? (double *)ar.get(nv3 * 8) : nullptr;
    int32_t *d_tri = (int32_t *)ar.get(nt3 * 4);
    if (ar.rc) return ar.rc;
    if ((rc = tsdf_mesh_emit(vol, W, d_vert, d_col, d_tri)) || (rc = r3d_download(ctx, vertices, d_vert, nv3)) ||
        (rc = r3d_download(ctx, colors, d_col, color ? nv3 : 0)) || (rc = r3d_download(ctx, triangles, d_tri, nt3)))
        return rc;
    R3D_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return R3D_OK;
}

int r3d_mesh_from_volume_dev(r3d_ctx *ctx, r3d_tsdf *vol, int64_t cap_vertices, int64_t cap_triangles, double *d_vertices, double *d_colors,
                             int32_t *d_triangles, int64_t *out_nv, int64_t *out_nt) {
    R3D_ROCTX_RANGE("r3d_mesh_from_volume_dev");
    if (!ctx) return R3D_E_BADARG;
    if (int rc = tsdf_mesh_args_ok(ctx, vol, cap_vertices, cap_triangles, d_vertices, d_colors, d_triangles, out_nv, out_nt)) return rc;
    R3D_HIP(ctx, hipSetDevice(ctx->device));
    DevArena ar(ctx);
    TsdfMeshWork W;
    int rc;
    if ((rc = tsdf_mesh_count(vol, ar, W, out_nv, out_nt))) return rc;
    if ((cap_vertices > 0 || cap_triangles > 0) && (W.total[0] > 0 || W.total[1] > 0) &&
        ((rc = tsdf_mesh_fits(ctx, ar, W, cap_vertices, cap_triangles)) || (rc = tsdf_mesh_emit(vol, W, d_vertices, d_colors, d_triangles))))
        return rc;
    R3D_HIP(ctx, hipStreamSynchronize(ctx->stream));   // the emitting kernels read arena buffers the next call may hand out again
    return R3D_OK;
}

int r3d_debug_volume_load_units(r3d_ctx *ctx, r3d_tsdf *vol, int64_t n, const int32_t *idx3, const float *tsdf, const float *weight, const double *colour) {
    R3D_ROCTX_RANGE("r3d_debug_volume_load_units");
    if (!ctx) return R3D_E_BADARG;
    if (int rc = tsdf_vol_ok(ctx, vol, "debug_volume_load_units")) return rc;
    const bool color = vol->prm.color_type == R3D_TSDF_COLOR_RGB8;
    if (n < 0 || n > (1 << 22) || (n > 0 && (!idx3 || !tsdf || !weight || (color && !colour))))
        return r3d_fail(ctx, R3D_E_BADARG, "debug_volume_load_units: a missing array, a negative count or more than 2^22 units");
    std::vector<unsigned long long> keys((size_t)n);
    for (int64_t i = 0; i < n; i++) {
        const int32_t *u = idx3 + i * 3;
        for (int k = 0; k < 3; k++)
            if (u[k] < -TSDF_IDX_LIMIT || u[k] >= TSDF_IDX_LIMIT)
                return r3d_fail(ctx, R3D_E_BADARG, "debug_volume_load_units: unit %lld has an index outside +-2^20", (long long)i);
        keys[(size_t)i] = tsdf_pack(u[0], u[1], u[2]);
    }
    {
        std::vector<unsigned long long> sorted(keys);
        std::sort(sorted.begin(), sorted.end());
        if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end())
            return r3d_fail(ctx, R3D_E_BADARG, "debug_volume_load_units: a unit index occurs twice");
    }
    R3D_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    if (n > vol->cap) {
        if (int rc = tsdf_resize(vol, (int)n)) {   // nothing of the volume has changed yet; the table may have been cleared
            const std::string why = ctx->err;
            (void)tsdf_clear_table(vol);
            ctx->err = why;
            return rc;
        }
        vol->growths++;
    }
    const size_t used = (size_t)n * TSDF_UNIT, old_used = (size_t)vol->n_units * TSDF_UNIT;
    if (n) {
        R3D_HIP(ctx, hipMemcpyAsync(vol->unit_keys.p, keys.data(), (size_t)n * 8, hipMemcpyHostToDevice, st));
        R3D_HIP(ctx, hipMemcpyAsync(vol->tsdf.p, tsdf, used * 4, hipMemcpyHostToDevice, st));
        R3D_HIP(ctx, hipMemcpyAsync(vol->weight.p, weight, used * 4, hipMemcpyHostToDevice, st));
        if (color)
            for (int ch = 0; ch < 3; ch++)   // host rows [unit][channel][4096] -> plane ch
                R3D_HIP(ctx, hipMemcpy2DAsync(vol->c[ch].p, TSDF_UNIT * 8, colour + (size_t)ch * TSDF_UNIT, 3 * TSDF_UNIT * 8, TSDF_UNIT * 8, (size_t)n,
                                              hipMemcpyHostToDevice, st));
    }
    if (old_used > used) {   // pool blocks past the units are zero, as k_tsdf_assign expects
        R3D_HIP(ctx, hipMemsetAsync((float *)vol->tsdf.p + used, 0, (old_used - used) * 4, st));
        R3D_HIP(ctx, hipMemsetAsync((float *)vol->weight.p + used, 0, (old_used - used) * 4, st));
        if (color)
            for (auto &p : vol->c) R3D_HIP(ctx, hipMemsetAsync((double *)p.p + used, 0, (old_used - used) * 8, st));
    }
    vol->n_units = (int)n;
    if (int rc = tsdf_clear_table(vol)) return rc;
    R3D_HIP(ctx, hipStreamSynchronize(st));   // the host arrays are the caller's again
    return R3D_OK;
}

int r3d_debug_mc_table(int8_t *tri256x16) {
    if (!tri256x16) return R3D_E_BADARG;
    memcpy(tri256x16, TSDF_MC_TRI, sizeof(TSDF_MC_TRI));
    return R3D_OK;
}

}  // extern "C"
