// sgm.hip -- semi-global block matching (3-way, and MODE_HH: k_hh_path / sgm_run_hh) for gfx950, hand-written for 64-wide wavefronts.
//
// Replaces cv2.StereoSGBM(mode=MODE_SGBM_3WAY).compute (reference call sites: Calib_depth/depth2.py:146-158,251
// and the other depth*.py files); the arithmetic restated here is OpenCV's stereosgbm.cpp as pinned down in
// oracle/sgbm3way.c (every QUIRK listed there is reproduced bit for bit).
//
// Data layout in HBM (all int16 unless noted; "dp" = the smallest of 32 / 64 / 128 / 256 / 512 slots that holds D; w1 = maxX1-minX1):
//   rec_l/rec_r  uint2 [cn][h][w]   per pixel and channel: (g, g_lo, g_hi, i | i_lo, i_hi, 0, 0): prefiltered gradient, raw
//                                   intensity and their Birchfield-Tomasi half-pixel intervals (cn = 1 grey, 3 colour)
//   cost         [h][w1][dp]        aggregated block cost C (blockSize x blockSize box of the BT pixel cost, summed over the
//                                   channels: k_cost2 runs once per channel, channels 1 and 2 add to what is stored)
//   cspec        [3][SH2][w1][dp]   C of the first SH2 rows of stripes 1..3 (box replicated at the stripe top)
//   hsum         [h][w1][dp]        L_left + L_right
//   raw / mins   [h][w]             WTA disparity (x16, before LR check) and its aggregated cost
// Lane mapping of every volume kernel: a disparity vector of dp entries lies on LPC adjacent lanes, NPL packed int16x2 registers
// (2*NPL consecutive disparities) per lane, dp = 2*NPL*LPC, so a wave holds 64/LPC vectors (rows, columns or lines) and the
// d-1 / d+1 neighbours come from one DPP shift each way ("Generic lane mapping" below).
// Pipeline of a MODE_SGBM_3WAY call (sgm_run_impl): k_prefilter -> k_cost2 (once per channel) -> k_hscan2 -> k_vscan2 (vertical
// path + winner-take-all) -> k_lrcheck -> (k_tiny_assemble) -> k_median3 -> (speckle filter).
#include <limits.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <initializer_list>
#include <vector>

#include "r3d_internal.h"

namespace {

typedef short s16x2 __attribute__((ext_vector_type(2)));
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));

constexpr int PADPK = 0x7fff7fff;  // SHRT_MAX in both halves: the d=-1 / d=D padding of every path buffer

__device__ __forceinline__ s16x2 as_s(int v) { return __builtin_bit_cast(s16x2, v); }
__device__ __forceinline__ u16x2 as_u(int v) { return __builtin_bit_cast(u16x2, v); }
__device__ __forceinline__ int as_i(s16x2 v) { return __builtin_bit_cast(int, v); }
__device__ __forceinline__ int as_i(u16x2 v) { return __builtin_bit_cast(int, v); }
__device__ __forceinline__ int pk_add(int a, int b) { return as_i(as_s(a) + as_s(b)); }
__device__ __forceinline__ int pk_sub(int a, int b) { return as_i(as_s(a) - as_s(b)); }
// Both halves known not to carry / borrow into each other (block costs: at most 121 * 189 = 22 869 per half): ONE 32-bit add, which
// gfx950 issues in ~2.5 cycles per wave against ~4.4 for v_pk_add_u16 (tools/micro/valu_rate.hip); same bits.
__device__ __forceinline__ int pk_add_nc(int a, int b) { return (int)((unsigned)a + (unsigned)b); }
__device__ __forceinline__ int pk_sub_nb(int a, int b) { return (int)((unsigned)a - (unsigned)b); }
__device__ __forceinline__ int pk_add_sat(int a, int b) { return as_i(__builtin_elementwise_add_sat(as_s(a), as_s(b))); }
__device__ __forceinline__ int pk_min(int a, int b) { return as_i(__builtin_elementwise_min(as_s(a), as_s(b))); }
__device__ __forceinline__ int pk_umax(int a, int b) { return as_i(__builtin_elementwise_max(as_u(a), as_u(b))); }
__device__ __forceinline__ int pk_umin(int a, int b) { return as_i(__builtin_elementwise_min(as_u(a), as_u(b))); }
__device__ __forceinline__ int pk_usub_sat(int a, int b) { return as_i(__builtin_elementwise_sub_sat(as_u(a), as_u(b))); }
__device__ __forceinline__ int pk_dup(int v) { return (v & 0xffff) | (v << 16); }
__device__ __forceinline__ int lo16(int v) { return (int)(short)(v & 0xffff); }
__device__ __forceinline__ int hi16(int v) { return v >> 16; }

// lane i receives lane i-1 (lane 0 keeps `fill`) / lane i+1 (lane 63 keeps `fill`)
__device__ __forceinline__ int wave_shr1(int v, int fill) { return __builtin_amdgcn_update_dpp(fill, v, 0x138, 0xf, 0xf, false); }
__device__ __forceinline__ int wave_shl1(int v, int fill) { return __builtin_amdgcn_update_dpp(fill, v, 0x130, 0xf, 0xf, false); }

// butterfly all-reduce over the 64 lanes: every lane ends with the result (xor 1, 2 via quad_perm; 4, 8 via
// row_half_mirror / row_mirror; 16, 32 via the gfx950 permlane swaps)
#define R3D_BUTTERFLY(OP)                                                                   \
    v = OP(v, (T)__builtin_amdgcn_update_dpp((int)v, (int)v, 0xB1, 0xf, 0xf, false));       \
    v = OP(v, (T)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x4E, 0xf, 0xf, false));       \
    v = OP(v, (T)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x141, 0xf, 0xf, false));      \
    v = OP(v, (T)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x140, 0xf, 0xf, false));      \
    { auto r = __builtin_amdgcn_permlane16_swap((unsigned)v, (unsigned)v, false, false); v = OP((T)r[0], (T)r[1]); } \
    { auto r = __builtin_amdgcn_permlane32_swap((unsigned)v, (unsigned)v, false, false); v = OP((T)r[0], (T)r[1]); }
__device__ __forceinline__ int wave_allmin_i32(int v) { typedef int T; R3D_BUTTERFLY(min) return v; }
__device__ __forceinline__ unsigned wave_allmin_u32(unsigned v) { typedef unsigned T; R3D_BUTTERFLY(min) return v; }
__device__ __forceinline__ int wave_allmax_i32(int v) { typedef int T; R3D_BUTTERFLY(max) return v; }

// ---------------------------------------------------------------------------------------------------------
// One SGM path step for one disparity vector (OpenCV accumulateCostsLeftTop / accumulateCostsRight):
//   L[d] = C[d] + min(Lp[d], Lp[d-1]+P1, Lp[d+1]+P1, minp+P2) - (minp+P2),   Lp[-1] = Lp[D] = SHRT_MAX
// P holds Lp on entry and L on exit; minp (wave-uniform) holds min_d Lp on entry and min_d L on exit.
// This wave-wide form (one vector of 128*NP disparities per wave) and sgm_step_dual are the definitions k_selftest holds the
// generic forms against; the kernels use sgm_step_g / sgm_step_dual_g.
// The packed adds cannot overflow inside the envelope checked on the host (C <= 16383, P2 <= 16383); the
// +P1 on the SHRT_MAX padding saturates (v_pk_add_i16 clamp), which never wins the min.
template <int NP>
__device__ __forceinline__ void sgm_step(int (&P)[NP], int &minp, const int (&C)[NP], int P1pk, int P2, bool lane_valid) {
    const int mp2 = pk_dup(minp + P2);
    const int up = wave_shr1(P[NP - 1], PADPK);  // lane-1's highest pair
    const int dn = wave_shl1(P[0], PADPK);       // lane+1's lowest pair
    int Q[NP];
    int m32 = 0x7fff;
#pragma unroll
    for (int j = 0; j < NP; j++) {
        const int below = j == 0 ? up : P[j - 1];
        const int above = j == NP - 1 ? dn : P[j + 1];
        const int A = __builtin_amdgcn_alignbit(P[j], below, 16);  // (L[d-1]) for both halves
        const int B = __builtin_amdgcn_alignbit(above, P[j], 16);  // (L[d+1]) for both halves
        const int nb = pk_add_sat(pk_min(A, B), P1pk);
        const int m = pk_min(pk_min(P[j], mp2), nb);
        int q = pk_add(C[j], pk_sub(m, mp2));
        q = lane_valid ? q : PADPK;
        Q[j] = q;
        m32 = min(m32, min(lo16(q), hi16(q)));
    }
#pragma unroll
    for (int j = 0; j < NP; j++) P[j] = Q[j];
    minp = wave_allmin_i32(m32);
}

// ---------------------------------------------------------------------------------------------------------
// Generic lane mapping of the volume kernels: a disparity vector of DP = 2*NPL*LPC entries is spread over LPC adjacent lanes,
// NPL packed registers (2*NPL consecutive disparities) per lane, so one wave holds 64/LPC independent vectors.
// Cross-lane work (2 DPP shifts + log2(LPC) butterfly stages) is amortised over NPL registers.
template <int LPC>
__device__ __forceinline__ int grp_shr1(int v, int fill, bool first) {  // lane i <- lane i-1 inside its LPC-lane group
    if constexpr (LPC == 1) return fill;
    else if constexpr (LPC == 64) return __builtin_amdgcn_update_dpp(fill, v, 0x138, 0xf, 0xf, false);
    else if constexpr (LPC == 32) { int t = __builtin_amdgcn_update_dpp(fill, v, 0x138, 0xf, 0xf, false); return first ? fill : t; }
    else { int t = __builtin_amdgcn_update_dpp(fill, v, 0x111, 0xf, 0xf, false); return (LPC < 16 && first) ? fill : t; }
}
template <int LPC>
__device__ __forceinline__ int grp_shl1(int v, int fill, bool last) {   // lane i <- lane i+1 inside its group
    if constexpr (LPC == 1) return fill;
    else if constexpr (LPC == 64) return __builtin_amdgcn_update_dpp(fill, v, 0x130, 0xf, 0xf, false);
    else if constexpr (LPC == 32) { int t = __builtin_amdgcn_update_dpp(fill, v, 0x130, 0xf, 0xf, false); return last ? fill : t; }
    else { int t = __builtin_amdgcn_update_dpp(fill, v, 0x101, 0xf, 0xf, false); return (LPC < 16 && last) ? fill : t; }
}
// all-reduce min inside each LPC-lane group; `old` = identity so that the DPP move folds into v_min_i32_dpp
template <int LPC>
__device__ __forceinline__ int grp_allmin(int v) {
    if constexpr (LPC >= 2) v = min(v, __builtin_amdgcn_update_dpp(0x7fffffff, v, 0xB1, 0xf, 0xf, false));
    if constexpr (LPC >= 4) v = min(v, __builtin_amdgcn_update_dpp(0x7fffffff, v, 0x4E, 0xf, 0xf, false));
    if constexpr (LPC >= 8) v = min(v, __builtin_amdgcn_update_dpp(0x7fffffff, v, 0x141, 0xf, 0xf, false));
    if constexpr (LPC >= 16) v = min(v, __builtin_amdgcn_update_dpp(0x7fffffff, v, 0x140, 0xf, 0xf, false));
    if constexpr (LPC >= 32) { auto r = __builtin_amdgcn_permlane16_swap((unsigned)v, (unsigned)v, false, false); v = min((int)r[0], (int)r[1]); }
    if constexpr (LPC >= 64) { auto r = __builtin_amdgcn_permlane32_swap((unsigned)v, (unsigned)v, false, false); v = min((int)r[0], (int)r[1]); }
    return v;
}
template <int LPC>
__device__ __forceinline__ int grp_allsum(int v) {
    if constexpr (LPC >= 2) v += __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xf, 0xf, false);
    if constexpr (LPC >= 4) v += __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xf, 0xf, false);
    if constexpr (LPC >= 8) v += __builtin_amdgcn_update_dpp(0, v, 0x141, 0xf, 0xf, false);
    if constexpr (LPC >= 16) v += __builtin_amdgcn_update_dpp(0, v, 0x140, 0xf, 0xf, false);
    if constexpr (LPC >= 32) { auto r = __builtin_amdgcn_permlane16_swap((unsigned)v, (unsigned)v, false, false); v = (int)r[0] + (int)r[1]; }
    if constexpr (LPC >= 64) { auto r = __builtin_amdgcn_permlane32_swap((unsigned)v, (unsigned)v, false, false); v = (int)r[0] + (int)r[1]; }
    return v;
}

// same recurrence as sgm_step, generic mapping; minp is uniform inside a group.  Critical path per step:
// add P2 -> pk_min -> pk_min -> pk_add -> (pk_min tree) -> sdwa min -> log2(LPC) butterfly stages.
template <int NPL, int LPC, bool PADDED = true>
__device__ __forceinline__ void sgm_step_g(int (&P)[NPL], int &minp, const int (&C)[NPL], int P1pk, int P2, bool first, bool last,
                                           bool lane_valid) {
    const short m16 = (short)(minp + P2);
    const int mp2 = as_i((s16x2){m16, m16});      // splat: folded into op_sel by the compiler
    const int up = grp_shr1<LPC>(P[NPL - 1], PADPK, first);
    const int dn = grp_shl1<LPC>(P[0], PADPK, last);
    // Stage by stage across all NPL registers ("breadth first"): on gfx950 a packed (VOP3P) result needs one wait state
    // before a dependent VALU read, and the compiler fills it with s_nop instead of independent work when the source is
    // written register by register; in this order every dependent pair is NPL instructions apart.
    int Q[NPL], t1[NPL], t3[NPL], cm[NPL];
#pragma unroll
    for (int j = 0; j < NPL; j++) {
        const int below = j == 0 ? up : P[j - 1];
        const int above = j == NPL - 1 ? dn : P[j + 1];
        const int A = __builtin_amdgcn_alignbit(P[j], below, 16);
        const int B = __builtin_amdgcn_alignbit(above, P[j], 16);
        t1[j] = pk_min(A, B);
    }
#pragma unroll
    for (int j = 0; j < NPL; j++) cm[j] = pk_sub(C[j], mp2);  // independent of the min chain
#pragma unroll
    for (int j = 0; j < NPL; j++) t3[j] = pk_min(P[j], mp2);
#pragma unroll
    for (int j = 0; j < NPL; j++) t1[j] = pk_add_sat(t1[j], P1pk);
#pragma unroll
    for (int j = 0; j < NPL; j++) t3[j] = pk_min(t3[j], t1[j]);
#pragma unroll
    for (int j = 0; j < NPL; j++) {
        const int q = pk_add(cm[j], t3[j]);
        Q[j] = (!PADDED || lane_valid) ? q : PADPK;
    }
    // balanced min tree (a linear chain would pay the wait state at every step)
    int mt[NPL];
#pragma unroll
    for (int j = 0; j < NPL; j++) mt[j] = Q[j];
#pragma unroll
    for (int w = NPL / 2; w >= 1; w /= 2) {
#pragma unroll
        for (int j = 0; j < w; j++) mt[j] = pk_min(mt[j], mt[j + w]);
    }
    const int m = mt[0];
#pragma unroll
    for (int j = 0; j < NPL; j++) P[j] = Q[j];
    minp = grp_allmin<LPC>(min(lo16(m), hi16(m)));
}

// Two independent chains (A, B) of the wave-wide mapping (NPL = 1, LPC = 64) advanced in lockstep: their per-lane minima
// travel through ONE packed butterfly (lo16 = A, hi16 = B; v_pk_min_i16 cannot take a DPP modifier, so each of the
// four row stages is mov_dpp + pk_min), which both shortens the instruction stream and hard-wires the interleave that
// the scheduler does not find by itself.  minAB holds (min A | min B << 16).
__device__ __forceinline__ int pk_allmin64(int v) {
    // every lane has a source in these four permutations, so the DPP move needs no `old` value (no extra copy)
    v = pk_min(v, __builtin_amdgcn_mov_dpp(v, 0xB1, 0xf, 0xf, true));
    v = pk_min(v, __builtin_amdgcn_mov_dpp(v, 0x4E, 0xf, 0xf, true));
    v = pk_min(v, __builtin_amdgcn_mov_dpp(v, 0x141, 0xf, 0xf, true));
    v = pk_min(v, __builtin_amdgcn_mov_dpp(v, 0x140, 0xf, 0xf, true));
    { auto r = __builtin_amdgcn_permlane16_swap((unsigned)v, (unsigned)v, false, false); v = pk_min((int)r[0], (int)r[1]); }
    { auto r = __builtin_amdgcn_permlane32_swap((unsigned)v, (unsigned)v, false, false); v = pk_min((int)r[0], (int)r[1]); }
    return v;
}
template <bool PADDED>
__device__ __forceinline__ void sgm_step_dual(int &PA, int &PB, int &minAB, int CA, int CB, int P1pk, int P2pk, bool lane_valid) {
    const s16x2 m = as_s(pk_add(minAB, P2pk));
    const int mp2A = as_i((s16x2){m.x, m.x}), mp2B = as_i((s16x2){m.y, m.y});
    const int upA = wave_shr1(PA, PADPK), upB = wave_shr1(PB, PADPK);
    const int dnA = wave_shl1(PA, PADPK), dnB = wave_shl1(PB, PADPK);
    const int nbA = pk_add_sat(pk_min(__builtin_amdgcn_alignbit(PA, upA, 16), __builtin_amdgcn_alignbit(dnA, PA, 16)), P1pk);
    const int nbB = pk_add_sat(pk_min(__builtin_amdgcn_alignbit(PB, upB, 16), __builtin_amdgcn_alignbit(dnB, PB, 16)), P1pk);
    const int cmA = pk_sub(CA, mp2A), cmB = pk_sub(CB, mp2B);
    int qA = pk_add(cmA, pk_min(pk_min(PA, mp2A), nbA));
    int qB = pk_add(cmB, pk_min(pk_min(PB, mp2B), nbB));
    if (PADDED) { qA = lane_valid ? qA : PADPK; qB = lane_valid ? qB : PADPK; }
    PA = qA; PB = qB;
    // (lo A | lo B << 16) vs (hi A | hi B << 16)
    const int lo = __builtin_amdgcn_perm(qB, qA, 0x05040100), hi = __builtin_amdgcn_perm(qB, qA, 0x07060302);
    minAB = pk_allmin64(pk_min(lo, hi));
}

// packed (two int16 lanes) all-reduce min inside each LPC-lane group
template <int LPC>
__device__ __forceinline__ int pk_grp_allmin(int v) {
    if constexpr (LPC >= 2) v = pk_min(v, __builtin_amdgcn_mov_dpp(v, 0xB1, 0xf, 0xf, true));
    if constexpr (LPC >= 4) v = pk_min(v, __builtin_amdgcn_mov_dpp(v, 0x4E, 0xf, 0xf, true));
    if constexpr (LPC >= 8) v = pk_min(v, __builtin_amdgcn_mov_dpp(v, 0x141, 0xf, 0xf, true));
    if constexpr (LPC >= 16) v = pk_min(v, __builtin_amdgcn_mov_dpp(v, 0x140, 0xf, 0xf, true));
    if constexpr (LPC >= 32) { auto r = __builtin_amdgcn_permlane16_swap((unsigned)v, (unsigned)v, false, false); v = pk_min((int)r[0], (int)r[1]); }
    if constexpr (LPC >= 64) { auto r = __builtin_amdgcn_permlane32_swap((unsigned)v, (unsigned)v, false, false); v = pk_min((int)r[0], (int)r[1]); }
    return v;
}
// two independent chains (A, B) of the generic mapping advanced in lockstep, sharing one packed butterfly
template <int NPL, int LPC, bool PADDED>
__device__ __forceinline__ void sgm_step_dual_g(int (&PA)[NPL], int (&PB)[NPL], int &minAB, const int (&CA)[NPL], const int (&CB)[NPL],
                                                int P1pk, int P2pk, bool first, bool last, bool lane_valid) {
    const s16x2 m = as_s(pk_add(minAB, P2pk));
    const int mp2A = as_i((s16x2){m.x, m.x}), mp2B = as_i((s16x2){m.y, m.y});
    const int upA = grp_shr1<LPC>(PA[NPL - 1], PADPK, first), upB = grp_shr1<LPC>(PB[NPL - 1], PADPK, first);
    const int dnA = grp_shl1<LPC>(PA[0], PADPK, last), dnB = grp_shl1<LPC>(PB[0], PADPK, last);
    int QA[NPL], QB[NPL];
#pragma unroll
    for (int j = 0; j < NPL; j++) {
        const int belowA = j == 0 ? upA : PA[j - 1], aboveA = j == NPL - 1 ? dnA : PA[j + 1];
        const int belowB = j == 0 ? upB : PB[j - 1], aboveB = j == NPL - 1 ? dnB : PB[j + 1];
        const int nbA = pk_add_sat(pk_min(__builtin_amdgcn_alignbit(PA[j], belowA, 16), __builtin_amdgcn_alignbit(aboveA, PA[j], 16)), P1pk);
        const int nbB = pk_add_sat(pk_min(__builtin_amdgcn_alignbit(PB[j], belowB, 16), __builtin_amdgcn_alignbit(aboveB, PB[j], 16)), P1pk);
        int qA = pk_add(pk_sub(CA[j], mp2A), pk_min(pk_min(PA[j], mp2A), nbA));
        int qB = pk_add(pk_sub(CB[j], mp2B), pk_min(pk_min(PB[j], mp2B), nbB));
        if (PADDED) { qA = lane_valid ? qA : PADPK; qB = lane_valid ? qB : PADPK; }
        QA[j] = qA; QB[j] = qB;
    }
    int mA = QA[0], mB = QB[0];
#pragma unroll
    for (int j = 1; j < NPL; j++) { mA = pk_min(mA, QA[j]); mB = pk_min(mB, QB[j]); }
#pragma unroll
    for (int j = 0; j < NPL; j++) { PA[j] = QA[j]; PB[j] = QB[j]; }
    const int lo = __builtin_amdgcn_perm(mB, mA, 0x05040100), hi = __builtin_amdgcn_perm(mB, mA, 0x07060302);
    minAB = pk_grp_allmin<LPC>(pk_min(lo, hi));
}

// trunc(n / d) for d > 0, |n|, d < 2^23: float reciprocal estimate + exact integer correction
__device__ __forceinline__ int trunc_div_small(int n, int d) {
    int q = (int)((float)n * __builtin_amdgcn_rcpf((float)d));
    int r = n - q * d;
    if (n >= 0) { if (r < 0) q--; else if (r >= d) q++; }
    else { if (r > 0) q++; else if (r <= -d) q--; }
    return q;
}
// smallest integer T with T * a >= thr  (a > 0): S * a < thr  <=>  S < T
__device__ __forceinline__ int ceil_div_small(int thr, int a, float inv_a) {
    // |thr| < 2^23 and a <= 100: the float estimate is within one of the answer; two branch-free corrections each way (a
    // `while` here becomes a divergent loop with exec-mask branches in the middle of the row step)
    int q = (int)floorf((float)thr * inv_a);
    q += (q * a < thr) ? 1 : 0;
    q += (q * a < thr) ? 1 : 0;
    q -= ((q - 1) * a >= thr) ? 1 : 0;
    q -= ((q - 1) * a >= thr) ? 1 : 0;
    return q;
}

// ---------------------------------------------------------------------------------------------------------
// k_prefilter: per pixel, both images: clipped x-Sobel (calcPixelCostBT's `tab` lookup), raw intensity, and the
// half-pixel min/max intervals of both.  QUIRK: columns 0 and w-1 of both channels read ftzero.
// gradient(x, y) = clamp(2*(I[y][x+1]-I[y][x-1]) + (I[y-1][x+1]-I[y-1][x-1]) + (I[y+1][x+1]-I[y+1][x-1]), -ft, ft) + ft with rows
// clamped to the image; intensity = I[y][x].
__device__ __forceinline__ void bt_interval(int vm, int v, int vp, bool has_m, bool has_p, int &lo, int &hi) {
    int l = has_m ? (v + vm) / 2 : v, r = has_p ? (v + vp) / 2 : v;
    lo = min(min(l, r), v);
    hi = max(max(l, r), v);
}

__global__ void __launch_bounds__(256) k_fill_s16(int16_t *__restrict__ p, size_t n, int16_t v) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) p[i] = v;
}

// One workgroup per 256-pixel column segment and band of PF_ROWS rows: every source row is read once (260 columns incl.
// halo; a thread keeps the three rows of its column in registers and rolls them), the gradient / intensity pair of 258
// positions is computed from LDS, and each thread forms its pixel's two intervals from its neighbours' pairs.  All global
// loads use clamped coordinates (no branch around a load).
// CN (1 or 3): channels of the interleaved source images (img[y * ld + x * CN + c]).  blockIdx.z = 2 * c + side: channel c of
// every pixel is prefiltered on its own, as a grey image would be, into plane c of the record images (rec[c][h][w]).
#define PF_ROWS 8
template <int CN>
__global__ void __launch_bounds__(256) k_prefilter(const uint8_t *__restrict__ L, const uint8_t *__restrict__ R, int ld,
                                                   int W, int H, int ft, uint2 *__restrict__ recL, uint2 *__restrict__ recR) {
    __shared__ int raw[260];  // rows y-1 | y << 8 | y+1 << 16 at columns x0-2 .. x0+257
    __shared__ int gi[258];   // gradient | intensity << 8 at columns x0-1 .. x0+256
    const int t = threadIdx.x, x0 = blockIdx.x * 256, yb = blockIdx.y * PF_ROWS;
    const int side = CN == 1 ? blockIdx.z : blockIdx.z & 1, ch = CN == 1 ? 0 : blockIdx.z >> 1;
    const uint8_t *img = (side == 0 ? L : R) + ch;
    uint2 *rec = (side == 0 ? recL : recR) + (size_t)ch * W * H;
    const int xc = min(max(x0 - 2 + t, 0), W - 1), xe = min(max(x0 + 254 + (t & 3), 0), W - 1);
    auto px = [&](int yy, int xx) { return (int)img[(size_t)min(max(yy, 0), H - 1) * ld + xx * CN]; };
    int a = px(yb - 1, xc), r = px(yb, xc), ae = px(yb - 1, xe), re = px(yb, xe);
    int bn = px(yb + 1, xc), ben = px(yb + 1, xe);   // the row below, requested ONE iteration early (its round trip ran on the critical path of every row)
    const int x = x0 + t;
    const bool hm = x > 0, hp = x < W - 1;
    for (int y = yb; y < min(yb + PF_ROWS, H); y++) {
        const int b = bn, be = ben;
        bn = px(y + 2, xc); ben = px(y + 2, xe);
        raw[t] = a | (r << 8) | (b << 16);
        if (t < 4) raw[256 + t] = ae | (re << 8) | (be << 16);
        a = r; r = b; ae = re; re = be;
        __syncthreads();
        auto pair_at = [&](int j) {  // j: index into gi, column x0-1+j, raw index of that column = j+1
            const int xx = x0 - 1 + j;
            const int m = raw[j], c = raw[j + 1], p = raw[j + 2];
            const int s = (((p >> 8) & 255) - ((m >> 8) & 255)) * 2 + ((p & 255) - (m & 255)) + (((p >> 16) & 255) - ((m >> 16) & 255));
            int g = min(max(s, -ft), ft) + ft, i = (c >> 8) & 255;
            if (xx <= 0 || xx >= W - 1) { g = ft; i = ft; }
            gi[j] = g | (i << 8);
        };
        pair_at(t);
        if (t < 2) pair_at(256 + t);
        __syncthreads();
        if (x < W) {
            const int vm = gi[t], v = gi[t + 1], vp = gi[t + 2];
            int g0, g1, i0, i1;
            const int g = v & 255, i = v >> 8;
            bt_interval(vm & 255, g, vp & 255, hm, hp, g0, g1);
            bt_interval(vm >> 8, i, vp >> 8, hm, hp, i0, i1);
            rec[(size_t)y * W + x] = make_uint2((unsigned)g | (g0 << 8) | (g1 << 16) | (i << 24), (unsigned)i0 | (i1 << 8));
        }
    }
}

__device__ __forceinline__ int bt_cost_pk(int U, int U0, int U1, int V, int V0, int V1) {
    int c0 = pk_umax(pk_usub_sat(U, V1), pk_usub_sat(V0, U));
    int c1 = pk_umax(pk_usub_sat(V, U1), pk_usub_sat(U0, V));
    return pk_umin(c0, c1);
}

// ---------------------------------------------------------------------------------------------------------
// k_cost2: Birchfield-Tomasi pixel cost -> blockSize x blockSize box sum -> cost volume, on the vector pipes.
// Mapping: lane = (column g = lane / LPC, disparity chunk k = lane % LPC), 16 disparities (8 packed registers) per lane,
// CW = 64/LPC adjacent columns per wave, NWAVE waves per workgroup = one tile of TC = NWAVE*CW columns (2*SH2 of them
// halo) that marches DOWN a band of rows:
//   per row: (a) all threads stage the NEXT row's inputs into LDS: left records, and for the right image ready-made
//                packed pair words W_q[r] = q[r] | q[r-1] << 16 for the six BT quantities (no byte shuffles later);
//            (b) every lane evaluates the Birchfield-Tomasi cost of its 16 disparities (3 ds_read_b64 + 17 packed
//                VALU per register) and slides the VERTICAL box sum, whose 2*SH2+1 rows live in registers;
//            (c) vertical sums go to an LDS tile; one barrier; (d) each lane adds the 2*SH2+1 neighbouring columns
//                (ds_read_b128) and streams C to HBM, 2 KB contiguous per wave.
// Borders: columns clamp in cost coordinates, rows clamp to [clampTop, h-1] (replication, as the original).
// blockIdx.y: the first nMain blocks each own a band of BAND rows of the main volume; the last three own the first SH2 rows of
// stripes 1..3 (cspec), whose box is replicated at the stripe top.
// ACC (colour pairs, channels 1 and 2): the block cost of this launch's channel is ADDED to what the launches of the
// earlier channels left in cvol / cspec (read-add-store by the lane that stores; every launch covers the same entries).  The sum
// of the channels stays below 32768 per entry (derive_geom), so the one 32-bit add of two packed entries carries nothing across.
// TRACK then looks at the summed value: it is set on the last channel's launch only.
template <int LPC, int SH2, bool TRACK, int NWAVE, bool ACC = false>
__global__ void __launch_bounds__(NWAVE * 64) k_cost2(const uint2 *__restrict__ recL, const uint2 *__restrict__ recR, SgmGeom g,
                                                            int *__restrict__ cvol, int *__restrict__ cspec, int BAND, int nMain,
                                                            int *__restrict__ maxc, int tile0) {
    constexpr int NPL = 8, CW = 64 / LPC, TC = NWAVE * CW, TO = TC - 2 * SH2, DP = 16 * LPC, DPW = NPL * LPC;
    constexpr int R = 2 * SH2 + 1, NRR = TC + DP, NT = NWAVE * 64;
    // pair words: 6 dwords per right pixel, plus 8 dwords of padding after every 16 pixels: lanes of one column group
    // read records 16 apart (16*6 dwords = 32 mod 64 banks -> 4-way conflicts); with the pad the eight chunks land on
    // eight different multiples of 8 banks and the four column groups of a half-wave fill the gaps: conflict-free.
    // LPC = 32 (DP = 512): a half-wave (the 32 lanes one ds_read_b64 cycle serves) is ONE column group of 32 chunks, and a chunk
    // stride of 16*6 + 8 = 104 = 40 mod 64 banks only has 8 distinct positions (4-way conflicts).  A pad of 2 dwords makes the
    // stride 98 = 2 * 49: chunk c starts at bank pair 49*c mod 32, a permutation of the 32 pairs, so the 32 8-byte reads of a
    // half-wave cover the 64 banks exactly once (and every record stays 8-byte aligned).  By construction, not measured.
    constexpr int PAD = LPC == 32 ? 2 : 8;
    constexpr int SWN = NRR * 6 + (NRR / 16 + 1) * PAD;
    __shared__ int sW[2][SWN];            // right-image pair words of one row, double buffered
    __shared__ uint2 sL[2][TC];           // left records of one row
    __shared__ int sV[2][TC * DPW];       // vertical box sums of the tile, double buffered
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, k = lane % LPC, grp = lane / LPC;
    const int cl = w * CW + grp;                       // local column 0..TC-1
    // first OUTPUT cost column of the tile.  tile0 is always 0 (every launch covers the whole width): kept as an argument so that the
    // instruction stream equals the previous build's
    const int t0 = (blockIdx.x + tile0) * TO;
    const int xc = min(max(t0 - SH2 + cl, 0), g.W1 - 1);   // cost column this lane evaluates (replicated at the borders)
    const int x = xc + g.minX1;                        // image column
    const int r_base = max(t0 - SH2, 0) + g.minX1 - g.minD - (DP - 1);
    const int ri0 = min(max(x - g.minD - 16 * k - r_base, 15), NRR - 1);   // pair-word index of this lane's lowest disparity
    const size_t rowWords = (size_t)g.W1 * DPW;
    int y0, y1, clampTop;
    int *obase;
    if ((int)blockIdx.y < nMain) {
        y0 = blockIdx.y * BAND; y1 = min(y0 + BAND, g.H); clampTop = 0;
        obase = cvol + (size_t)y0 * rowWords;
    } else {
        const int n = blockIdx.y - nMain + 1;
        const int ss = max(min(n * g.stripe_sz - g.overlap, g.H), 0);
        y0 = ss; y1 = min(ss + SH2, g.H); clampTop = ss;
        obase = cspec + (size_t)(n - 1) * SH2 * rowWords;
    }
    if (y0 >= y1) return;
    auto crow = [&](int yy) { return min(max(yy, clampTop), g.H - 1); };

    // (a) staging of an image row: the raw records are fetched one iteration EARLY into registers (fetch), and turned
    // into LDS pair words one iteration later (commit), so the global-load latency is never waited for inside a row
    // One pair-word record per thread and pass: NREC = 1 up to DP = 256; DP = 512 has NRR = 16 + 512 = 528 records for its 512
    // threads, so the last 16 go through a second pass of the first 16 threads (two more uint2 in flight per thread).
    constexpr int NREC = (NRR + NT - 1) / NT;
    static_assert(NRR <= NREC * NT && NREC <= 2, "pair-word records per thread");
    uint2 pfL = make_uint2(0, 0), pfA[NREC], pfB[NREC];
#pragma unroll
    for (int q = 0; q < NREC; q++) pfA[q] = pfB[q] = make_uint2(0, 0);
    auto fetch = [&](int row) {
        const uint2 *lr = recL + (size_t)row * g.W, *rr = recR + (size_t)row * g.W;
        if (tid < TC) pfL = lr[min(max(t0 - SH2 + tid, 0), g.W1 - 1) + g.minX1];
#pragma unroll
        for (int q = 0; q < NREC; q++) {
            const int i = tid + q * NT;
            if (i < NRR) {
                const int r = r_base + i;
                pfA[q] = rr[min(max(r, 0), g.W - 1)];
                pfB[q] = rr[min(max(r - 1, 0), g.W - 1)];
            }
        }
    };
    auto commit = [&](int b) {
        if (tid < TC) sL[b][tid] = pfL;
#pragma unroll
        for (int q = 0; q < NREC; q++) {
            const int i = tid + q * NT;
            if (i < NRR) {
                const uint2 A = pfA[q], B = pfB[q];
                int *o = &sW[b][i * 6 + (i >> 4) * PAD];
                o[0] = __builtin_amdgcn_perm(B.x, A.x, 0x0c040c00); o[1] = __builtin_amdgcn_perm(B.x, A.x, 0x0c050c01);
                o[2] = __builtin_amdgcn_perm(B.x, A.x, 0x0c060c02); o[3] = __builtin_amdgcn_perm(B.x, A.x, 0x0c070c03);
                o[4] = __builtin_amdgcn_perm(B.y, A.y, 0x0c040c00); o[5] = __builtin_amdgcn_perm(B.y, A.y, 0x0c050c01);
            }
        }
    };
    // (b) BT pixel cost of this lane's 16 disparities from buffer b
    auto pixel_cost = [&](int b, int (&pix)[NPL]) {
        const uint2 lr = sL[b][cl];
        const int Ug = __builtin_amdgcn_perm(lr.x, lr.x, 0x0c000c00), Ug0 = __builtin_amdgcn_perm(lr.x, lr.x, 0x0c010c01);
        const int Ug1 = __builtin_amdgcn_perm(lr.x, lr.x, 0x0c020c02), Ui = __builtin_amdgcn_perm(lr.x, lr.x, 0x0c030c03);
        const int Ui0 = __builtin_amdgcn_perm(lr.y, lr.y, 0x0c000c00), Ui1 = __builtin_amdgcn_perm(lr.y, lr.y, 0x0c010c01);
#pragma unroll
        for (int j = 0; j < NPL; j++) {
            const int rj = ri0 - 2 * j;
            // three ds_read_b64 (banks mod 64, 2 LDS cycles each, conflict-free with the padding above).  Volatile keeps the compiler
            // from pairing two of them into ds_read2_b64, which is banked mod 32 in 16-lane groups: chunks k and k+4 then collide
            // (2-way) and the pair costs 16 LDS cycles instead of 4 -- the 31 % bank conflicts of the round-2/3 counters.
            typedef int v2i __attribute__((ext_vector_type(2)));
            typedef const volatile __attribute__((address_space(3))) v2i lds_v2i;   // (a plain volatile pointer would read through flat_load)
            lds_v2i *p = (lds_v2i *)&sW[b][rj * 6 + (rj >> 4) * PAD];
            const v2i a = p[0], bq = p[1], c = p[2];       // (Vg, Vg0) (Vg1, Vi) (Vi0, Vi1)
            const int cg = bt_cost_pk(Ug, Ug0, Ug1, a.x, a.y, bq.x);
            const int ci = bt_cost_pk(Ui, Ui0, Ui1, bq.y, c.x, c.y);
            pix[j] = pk_add_nc(cg, (ci >> 2) & 0x3fff3fff);
        }
    };

    // The vertical window (R rows of pixel costs, each <= 189 so stored as bytes: 4 registers per row) lives in
    // registers and is rotated by plain moves, which keeps the loop rolled and the register count predictable.
    int ring[R][NPL / 2], vs[NPL];
#pragma unroll
    for (int j = 0; j < NPL; j++) vs[j] = 0;
#pragma unroll
    for (int q = 0; q < R; q++)
#pragma unroll
        for (int j = 0; j < NPL / 2; j++) ring[q][j] = 0;
    const bool is_out = cl >= SH2 && cl < TC - SH2 && (t0 - SH2 + cl) < g.W1;
    int *optr = obase + (size_t)(t0 - SH2 + cl) * DPW + k * NPL;
    const int tile_x0 = t0 - SH2;
    int cmax = 0;   // TRACK: running maximum of every emitted block cost (exact-arithmetic envelope check on the host)
    fetch(crow(y0 - SH2));
    commit(0);
    fetch(crow(y0 - SH2 + 1));
    commit(1);
    fetch(crow(y0 - SH2 + 2));
    __syncthreads();
    // iteration t: row e = y0 - SH2 + t enters the window (inputs in buffer t&1, staged TWO iterations earlier);
    // from t = 2*SH2 on the window is full and output row y = e - SH2 is produced.  One barrier per iteration.
    // The staging of row t+2 sits right AFTER the barrier (buffer t&1 is free from there on), not before it: its wait for the
    // prefetched records is an s_waitcnt vmcnt(0) (the count cannot be known across the conditional stores), which also waits for
    // this wave's own stores of C -- issued a whole iteration earlier here, most of an iteration earlier in the old order, where
    // waves 0-2 stalled on them (~1.8 us of write latency against a 2.1 us iteration) and the other five at the barrier behind them
    // (DESIGN.md section 4).
    const int niter = (y1 - y0) + 2 * SH2;
#pragma unroll 1
    for (int t = 0; t < niter; t++) {
        const int b = t & 1;
        int pn[NPL];
        pixel_cost(b, pn);
#pragma unroll
        for (int j = 0; j < NPL / 2; j++) {
            const int old = ring[0][j];
            vs[2 * j] = pk_add_nc(pk_sub_nb(vs[2 * j], __builtin_amdgcn_perm(old, old, 0x0c010c00)), pn[2 * j]);
            vs[2 * j + 1] = pk_add_nc(pk_sub_nb(vs[2 * j + 1], __builtin_amdgcn_perm(old, old, 0x0c030c02)), pn[2 * j + 1]);
        }
#pragma unroll
        for (int q = 0; q + 1 < R; q++)
#pragma unroll
            for (int j = 0; j < NPL / 2; j++) ring[q][j] = ring[q + 1][j];
#pragma unroll
        for (int j = 0; j < NPL / 2; j++) ring[R - 1][j] = __builtin_amdgcn_perm(pn[2 * j + 1], pn[2 * j], 0x06040200);
        const bool outp = t >= 2 * SH2;
        if (outp) {
            // tile layout: column-major, inside a column the two 16-byte halves of all lanes are stored as two planes
            // whose order alternates with the column parity: conflict-free for the b128 write and the b128 reads below
            *(int4 *)&sV[b][cl * DPW + (DPW / 2) * (cl & 1) + 4 * k] = make_int4(vs[0], vs[1], vs[2], vs[3]);
            *(int4 *)&sV[b][cl * DPW + (DPW / 2) * ((cl & 1) ^ 1) + 4 * k] = make_int4(vs[4], vs[5], vs[6], vs[7]);
        }
        __syncthreads();
        commit(b);                                      // row t+2 (fetched during iteration t-1) into the buffer this iteration just read
        fetch(crow(y0 - SH2 + t + 3));                  // row t+3, consumed by the next iteration's commit
        const bool do_out = outp && is_out;
        int c[NPL];
#pragma unroll
        for (int j = 0; j < NPL; j++) c[j] = 0;
        if (do_out) {
#pragma unroll
            for (int i = -SH2; i <= SH2; i++) {
                const int col = min(max(tile_x0 + cl + i, 0), g.W1 - 1) - tile_x0;
                const int4 v0 = *(const int4 *)&sV[b][col * DPW + (DPW / 2) * (col & 1) + 4 * k];
                const int4 v1 = *(const int4 *)&sV[b][col * DPW + (DPW / 2) * ((col & 1) ^ 1) + 4 * k];
                c[0] = pk_add_nc(c[0], v0.x); c[1] = pk_add_nc(c[1], v0.y); c[2] = pk_add_nc(c[2], v0.z); c[3] = pk_add_nc(c[3], v0.w);
                c[4] = pk_add_nc(c[4], v1.x); c[5] = pk_add_nc(c[5], v1.y); c[6] = pk_add_nc(c[6], v1.z); c[7] = pk_add_nc(c[7], v1.w);
            }
        }
        if (do_out) {
            int *o = optr + (size_t)(t - 2 * SH2) * rowWords;
            if constexpr (ACC) {
                const int4 a0 = *(const int4 *)o, a1 = *(const int4 *)(o + 4);
                c[0] = pk_add_nc(c[0], a0.x); c[1] = pk_add_nc(c[1], a0.y); c[2] = pk_add_nc(c[2], a0.z); c[3] = pk_add_nc(c[3], a0.w);
                c[4] = pk_add_nc(c[4], a1.x); c[5] = pk_add_nc(c[5], a1.y); c[6] = pk_add_nc(c[6], a1.z); c[7] = pk_add_nc(c[7], a1.w);
            }
            *(int4 *)o = make_int4(c[0], c[1], c[2], c[3]);
            *(int4 *)(o + 4) = make_int4(c[4], c[5], c[6], c[7]);
            if (TRACK && 16 * k < g.D) {
#pragma unroll
                for (int j = 0; j < NPL; j++) cmax = pk_umax(cmax, c[j]);
            }
        }
    }
    if (TRACK) {
        const int m = wave_allmax_i32(max(cmax & 0xffff, (int)((unsigned)cmax >> 16)));
        if (lane == 0) atomicMax(maxc, m);
    }
}

// ---------------------------------------------------------------------------------------------------------
// k_hscan2: the two horizontal paths of 64 / LPC image rows per wave (LPC lanes x NPL packed registers per row), NO spill of L_left to HBM.
//   phase 1: forward chain over the row; the state entering every K-column segment is check-pointed (DP + 16 bytes per row);
//   phase 2: segments right-to-left: the segment's C values are loaded ONCE into registers, the forward chain is
//            recomputed from the checkpoint (L_left of the segment stays in registers), then the backward chain
//            runs over the same registers and streams L_left + L_right to HBM.
// HBM traffic per row: C read twice, sum written once, + 2 * (DP + 16) B * W1/K of checkpoints.
// A tail of W1 % K columns parks its L_left in the output row between the two phases (written forward, read back and replaced by
// the sum by the same lanes).
template <int NPL, int LPC, int K, bool PADDED>
__global__ void __launch_bounds__(64) k_hscan2(const int *__restrict__ cvol, int *__restrict__ hvol, int *__restrict__ ckpt, SgmGeom g) {
    // words per column, rows per wave; CKS: words of one checkpoint = the DP/2 packed words of L + its minimum, padded to 16 B.
    // Checkpoints are addressed by image row.
    constexpr int DPW = NPL * LPC, RPW = 64 / LPC, CKS = DPW + 4;
    const int lane = threadIdx.x, k = lane % LPC;
    const int yraw = blockIdx.x * RPW + lane / LPC;
    const bool row_ok = yraw < g.H;
    const int y = min(yraw, g.H - 1);
    const int *crow = cvol + (size_t)y * g.W1 * DPW + k * NPL;
    int *hrow = hvol + (size_t)y * g.W1 * DPW + k * NPL;
    const int W1 = g.W1, nfull = W1 / K, P1pk = pk_dup(g.P1), P2pk = pk_dup(g.P2);
    int *ckrow = ckpt + (size_t)yraw * (nfull + 1) * CKS, *ck = ckrow + k * NPL;
    const bool valid = 2 * NPL * k < g.D, first = k == 0, last = k == LPC - 1;
    int P[NPL], minp = 0;
    // four rotating cost buffers: a segment is requested two rounds (2*K steps) before its first use and is never
    // touched in between, so the loads stay in flight across whole rounds
    int c0[K][NPL], c1[K][NPL], c2[K][NPL], c3[K][NPL], llA[K][NPL], llB[K][NPL];
#pragma unroll
    for (int j = 0; j < NPL; j++) P[j] = valid ? 0 : PADPK;
    const int seg_hi = nfull;   // segments of the forward sweep (a local of its own: DESIGN.md section 7)
    auto load_seg = [&](int (&buf)[K][NPL], int sidx) {
        const int sc = min(max(sidx, 0), max(seg_hi - 1, 0));
        const int *p = crow + (size_t)sc * K * DPW;
#pragma unroll
        for (int u = 0; u < K; u++)
#pragma unroll
            for (int j = 0; j < NPL; j++) buf[u][j] = p[(size_t)u * DPW + j];
    };
    auto save_ck = [&](int sidx) {
#pragma unroll
        for (int j = 0; j < NPL; j++) ck[(size_t)sidx * CKS + j] = P[j];
        if (first) ckrow[(size_t)sidx * CKS + DPW] = minp;
    };
    auto load_ck = [&](int sidx) {
#pragma unroll
        for (int j = 0; j < NPL; j++) P[j] = ck[(size_t)sidx * CKS + j];
        minp = ckrow[(size_t)sidx * CKS + DPW];
    };
    auto store_sum = [&](int *dst, const int (&a)[NPL], const int (&b)[NPL]) {
        if (row_ok) {
#pragma unroll
            for (int j = 0; j < NPL; j++) dst[j] = pk_add(a[j], b[j]);
        }
    };
    // ---- phase 1: forward chain, checkpoint the state entering every segment
    auto fwd_round = [&](int (&cur)[K][NPL], int (&pre)[K][NPL], int sidx) {   // pre <- segment sidx+3
        load_seg(pre, sidx + 3);
        save_ck(sidx);
#pragma unroll
        for (int u = 0; u < K; u++) sgm_step_g<NPL, LPC, PADDED>(P, minp, cur[u], P1pk, g.P2, first, last, valid);
    };
    if (seg_hi > 0) {
        load_seg(c0, 0); load_seg(c1, 1); load_seg(c2, 2);
#pragma unroll 1
        for (int s0 = 0; s0 < seg_hi; s0 += 4) {
            fwd_round(c0, c3, s0);
            if (s0 + 1 < seg_hi) fwd_round(c1, c0, s0 + 1);
            if (s0 + 2 < seg_hi) fwd_round(c2, c1, s0 + 2);
            if (s0 + 3 < seg_hi) fwd_round(c3, c2, s0 + 3);
        }
    }
    // tail columns [nfull*K, W1): forward values parked in the output row (rows beyond the image park nothing: they
    // recompute nothing useful either, their results are never stored)
    for (int x = nfull * K; x < W1; x++) {
        int c[NPL];
#pragma unroll
        for (int j = 0; j < NPL; j++) c[j] = crow[(size_t)x * DPW + j];
        sgm_step_g<NPL, LPC, PADDED>(P, minp, c, P1pk, g.P2, first, last, valid);
        if (row_ok) {
#pragma unroll
            for (int j = 0; j < NPL; j++) hrow[(size_t)x * DPW + j] = P[j];
        }
    }
    // ---- phase 2: backward chain of segment s in lockstep with the recomputed forward chain of segment s-1
    int R[NPL], minr = 0;
#pragma unroll
    for (int j = 0; j < NPL; j++) R[j] = valid ? 0 : PADPK;
    for (int x = W1 - 1; x >= nfull * K; x--) {
        int c[NPL], l[NPL];
#pragma unroll
        for (int j = 0; j < NPL; j++) { c[j] = crow[(size_t)x * DPW + j]; l[j] = hrow[(size_t)x * DPW + j]; }
        sgm_step_g<NPL, LPC, PADDED>(R, minr, c, P1pk, g.P2, first, last, valid);
        store_sum(hrow + (size_t)x * DPW, l, R);
    }
    // The checkpoint a round starts from is requested one round EARLY (ckn / ckm): the memory queue retires in order, so a
    // checkpoint loaded where it is used waits for every load and store issued before it -- the round's own prefetch and
    // the previous round's 16 sum stores -- and with one wave per SIMD nothing hides that drain.
    int ckn[NPL], ckm = 0;
    auto fetch_ck = [&](int sidx) {
        const int sc = max(sidx, 0);
#pragma unroll
        for (int j = 0; j < NPL; j++) ckn[j] = ck[(size_t)sc * CKS + j];
        ckm = ckrow[(size_t)sc * CKS + DPW];
    };
    // round(s): A = costs of segment s (backward), B = costs of segment s-1 (forward), pre <- segment s-3;
    // LA = L_left of segment s (left by the round before), LB <- L_left of segment s-1.
    // SWAP: the rounds alternate the roles of llA and llB instead of copying llB into llA after every round (4 moves per
    // column).  Only where the six buffers overflow the 256 VGPRs anyway (DP = 128, K = 16: one wave per SIMD either way): in
    // the smaller layouts the copy lets the two buffers share registers, and the swap costs them their second wave per SIMD.
    constexpr bool SWAP = 6 * K * NPL > 256;
    auto bwd_round = [&](int (&A)[K][NPL], int (&B)[K][NPL], int (&pre)[K][NPL], int (&LA)[K][NPL], int (&LB)[K][NPL], int sidx) {
#pragma unroll
        for (int j = 0; j < NPL; j++) P[j] = ckn[j];           // the state entering segment s-1
        minp = ckm;
        fetch_ck(sidx - 2);
        load_seg(pre, sidx - 3);
        int *hp = hrow + (size_t)sidx * K * DPW;
        if (sidx > 0) {
            int mAB = (minr & 0xffff) | (minp << 16);
#pragma unroll
            for (int u = 0; u < K; u++) {
                sgm_step_dual_g<NPL, LPC, PADDED>(R, P, mAB, A[K - 1 - u], B[u], P1pk, P2pk, first, last, valid);
                store_sum(hp + (size_t)(K - 1 - u) * DPW, LA[K - 1 - u], R);
#pragma unroll
                for (int j = 0; j < NPL; j++) LB[u][j] = P[j];
            }
            minr = lo16(mAB);
        } else {
#pragma unroll
            for (int u = 0; u < K; u++) {
                sgm_step_g<NPL, LPC, PADDED>(R, minr, A[K - 1 - u], P1pk, g.P2, first, last, valid);
                store_sum(hp + (size_t)(K - 1 - u) * DPW, LA[K - 1 - u], R);
            }
        }
        if (!SWAP) {
#pragma unroll
            for (int u = 0; u < K; u++)
#pragma unroll
                for (int j = 0; j < NPL; j++) LA[u][j] = LB[u][j];
        }
    };
    if (nfull > 0) {
        load_seg(c0, nfull - 1); load_seg(c1, nfull - 2); load_seg(c2, nfull - 3);
        load_ck(nfull - 1);
        fetch_ck(nfull - 2);
#pragma unroll
        for (int u = 0; u < K; u++) {
            sgm_step_g<NPL, LPC, PADDED>(P, minp, c0[u], P1pk, g.P2, first, last, valid);
#pragma unroll
            for (int j = 0; j < NPL; j++) llA[u][j] = P[j];
        }
#pragma unroll 1
        for (int s = nfull - 1; s >= 0; s -= 4) {
            bwd_round(c0, c1, c3, llA, llB, s);
            if (s - 1 >= 0) bwd_round(c1, c2, c0, SWAP ? llB : llA, SWAP ? llA : llB, s - 1);
            if (s - 2 >= 0) bwd_round(c2, c3, c1, llA, llB, s - 2);
            if (s - 3 >= 0) bwd_round(c3, c0, c2, SWAP ? llB : llA, SWAP ? llA : llB, s - 3);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------
// k_vscan2: vertical path + winner-take-all with 16 disparities per lane (NPL = 8): LPC = DP/16 lanes per column,
// CPW = 64/LPC adjacent columns per wave, each column an independent chain inside its lane group.  Everything after
// the path step -- argmin (32-bit keys cost<<16|d, v_min3 tree + group butterfly), uniqueness (packed compare against
// the per-column threshold, counted), sub-pixel (the owner lane picks the winner's two neighbours out of its registers,
// a 3-stage butterfly shares them) -- is per-lane VALU work: no scalar unit traffic, no LDS, no barrier.
template <int NPL, int LPC>
__global__ void __launch_bounds__(64) k_vscan2(const int *__restrict__ cvol, const int *__restrict__ cspec,
                                               const int *__restrict__ hvol, SgmGeom g, float inv_a, int16_t *__restrict__ raw,
                                               int16_t *__restrict__ mins, int col0) {
    constexpr int CPW = 64 / LPC, DPW = NPL * LPC;  // columns per wave, words per column
    static_assert(NPL == 4 || NPL == 8 || NPL == 16, "one, two or four 16-byte loads per lane");
    const int lane = threadIdx.x, k = lane % LPC, grp = lane / LPC, n = blockIdx.y;
    const int xc = col0 + blockIdx.x * CPW + grp;   // cost column of this lane group; col0 is always 0, kept as tile0 is in k_cost2
    const bool col_ok = xc < g.W1;
    const size_t rowWords = (size_t)g.W1 * DPW;
    const int src_start = max(min(n * g.stripe_sz - g.overlap, g.H), 0);
    const int src_end = min((n + 1) * g.stripe_sz, g.H);
    const int out_start = min(n * g.stripe_sz, g.H);
    if (src_start >= src_end) return;
    const bool valid = 2 * NPL * k < g.D, first = k == 0, last = k == LPC - 1;
    const int P1pk = pk_dup(g.P1);
    const size_t off = (size_t)min(xc, g.W1 - 1) * DPW + k * NPL;
    const int a = 100 - g.uniq;
    int P[NPL], minp = 0;
#pragma unroll
    for (int j = 0; j < NPL; j++) P[j] = valid ? 0 : PADPK;
    int cc[NPL], hh[NPL], cn[NPL], hn[NPL];
    auto load_row = [&](int y, int (&cb)[NPL], int (&hb)[NPL]) {
        const int yy = min(y, src_end - 1);
        const int *cr = ((n > 0 && yy < src_start + g.SH2) ? cspec + ((size_t)(n - 1) * g.SH2 + (yy - src_start)) * rowWords
                                                             : cvol + (size_t)yy * rowWords) + off;
#pragma unroll
        for (int q = 0; q < NPL / 4; q++) {
            const int4 c0 = *(const int4 *)(cr + 4 * q);
            cb[4 * q] = c0.x; cb[4 * q + 1] = c0.y; cb[4 * q + 2] = c0.z; cb[4 * q + 3] = c0.w;
        }
        if (yy >= out_start) {
            const int *hr = hvol + (size_t)yy * rowWords + off;
#pragma unroll
            for (int q = 0; q < NPL / 4; q++) {
                const int4 h0 = *(const int4 *)(hr + 4 * q);
                hb[4 * q] = h0.x; hb[4 * q + 1] = h0.y; hb[4 * q + 2] = h0.z; hb[4 * q + 3] = h0.w;
            }
        }
    };
    auto process = [&](int y, int (&cb)[NPL], int (&hb)[NPL]) {
        sgm_step_g<NPL, LPC>(P, minp, cb, P1pk, g.P2, first, last, valid);
        if (y < out_start) return;
        int S[NPL];
        int key = 0x7fffffff;
#pragma unroll
        for (int j = 0; j < NPL; j++) {
            S[j] = pk_add_sat(hb[j], P[j]);
            const int d0 = 2 * NPL * k + 2 * j;
            const int k0 = (int)((unsigned)S[j] << 16) | d0;              // (cost of d0) << 16 | d0, signed order
            const int k1 = (S[j] & (int)0xffff0000) | (d0 + 1);
            key = min(key, min(k0, k1));
        }
        if (!valid) key = 0x7fffffff;
        key = grp_allmin<LPC>(key);
        const int best = key & 0xffff, minS = key >> 16;
        // the winner's neighbours S[best-1], S[best+1]: the lane that owns the disparity picks it out of its registers
        // with a select tree (the index is group-uniform, no LDS round trip, no barrier) and a 3-stage butterfly
        // hands it to the whole group
        auto fetch_s = [&](int d) -> int {
            const int j = (d >> 1) % NPL;
            int v;
            if constexpr (NPL == 16) {
                const bool b0 = j & 1, b1 = j & 2, b2 = j & 4;
                const int t0 = b0 ? S[1] : S[0], t1 = b0 ? S[3] : S[2], t2 = b0 ? S[5] : S[4], t3 = b0 ? S[7] : S[6];
                const int t4 = b0 ? S[9] : S[8], t5 = b0 ? S[11] : S[10], t6 = b0 ? S[13] : S[12], t7 = b0 ? S[15] : S[14];
                const int u0 = b1 ? t1 : t0, u1 = b1 ? t3 : t2, u2 = b1 ? t5 : t4, u3 = b1 ? t7 : t6;
                const int w0 = b2 ? u1 : u0, w1 = b2 ? u3 : u2;
                v = (j & 8) ? w1 : w0;
            } else if constexpr (NPL == 8) {
                const int t0 = (j & 1) ? S[1] : S[0], t1 = (j & 1) ? S[3] : S[2], t2 = (j & 1) ? S[5] : S[4], t3 = (j & 1) ? S[7] : S[6];
                const int u0 = (j & 2) ? t1 : t0, u1 = (j & 2) ? t3 : t2;
                v = (j & 4) ? u1 : u0;
            } else {
                const int t0 = (j & 1) ? S[1] : S[0], t1 = (j & 1) ? S[3] : S[2];
                v = (j & 2) ? t1 : t0;
            }
            const int val = (d & 1) ? hi16(v) : lo16(v);
            return grp_allmin<LPC>(((d / (2 * NPL)) == k) ? val : 0x7fffffff);
        };
        const int dm = max(best - 1, 0), dp = min(best + 1, g.D - 1);
        const int sm = fetch_s(dm), sp = fetch_s(dp);
        bool bad = false;
        if (g.uniq > 0) {
            // S*a < minS*100  <=>  S < T ; count the disparities below T, subtract those inside [best-1, best+1]
            const int T = ceil_div_small(minS * 100, a, inv_a);
            int cnt;
            if (T > 32767) cnt = valid ? 2 * NPL : 0;
            else {
                const int Tpk = pk_dup(max(T, -32768));
                int acc = 0;
#pragma unroll
                for (int j = 0; j < NPL; j++) {
                    const int diff = as_i(__builtin_elementwise_sub_sat(as_s(S[j]), as_s(Tpk)));   // < 0  <=>  S < T
                    acc = pk_sub(acc, as_i(as_s(diff) >> (s16x2){15, 15}));                        // += 1 per negative half
                }
                cnt = valid ? lo16(acc) + hi16(acc) : 0;
            }
            cnt = grp_allsum<LPC>(cnt);
            int win = (minS < T) ? 1 : 0;
            if (best > 0 && sm < T) win++;
            if (best < g.D - 1 && sp < T) win++;
            bad = cnt > win;
        }
        int dsp = g.invalid;
        if (!bad) {
            dsp = best * 16;
            if (0 < best && best < g.D - 1) {
                const int den = max(sm + sp - 2 * minS, 1);
                dsp += trunc_div_small((sm - sp) * 16 + den, den * 2);
            }
            dsp += g.minD * 16;
        }
        if (first && col_ok) {
            const size_t o = (size_t)y * g.W + g.minX1 + xc;
            raw[o] = (int16_t)dsp;
            mins[o] = (int16_t)minS;
        }
    };
    // four row buffers in rotation: a row is requested three rows (~3 x 900 cycles) before it is consumed
    int c2[NPL], h2[NPL], c3[NPL], h3[NPL];
    load_row(src_start, cc, hh);
    load_row(src_start + 1, cn, hn);
    load_row(src_start + 2, c2, h2);
#pragma unroll 1
    for (int y = src_start; y < src_end; y += 4) {
        load_row(y + 3, c3, h3);
        process(y, cc, hh);
        load_row(y + 4, cc, hh);
        if (y + 1 < src_end) process(y + 1, cn, hn);
        load_row(y + 5, cn, hn);
        if (y + 2 < src_end) process(y + 2, c2, h2);
        load_row(y + 6, c2, h2);
        if (y + 3 < src_end) process(y + 3, c3, h3);
    }
}

// ---------------------------------------------------------------------------------------------------------
// Winner-take-all + uniqueness + sub-pixel of one disparity vector held in registers in the generic mapping (the arithmetic
// of k_vscan2's row step as a function; group-uniform results; no LDS, no barrier).
template <int NPL, int LPC>
__device__ __forceinline__ void wta_regs(const int (&S)[NPL], int k, bool valid, const SgmGeom &g, int a, float inv_a, int &dsp_out,
                                         int &minS_out) {
    int key = 0x7fffffff;
#pragma unroll
    for (int j = 0; j < NPL; j++) {
        const int d0 = 2 * NPL * k + 2 * j;
        const int k0 = (int)((unsigned)S[j] << 16) | d0;
        const int k1 = (S[j] & (int)0xffff0000) | (d0 + 1);
        key = min(key, min(k0, k1));
    }
    if (!valid) key = 0x7fffffff;
    key = grp_allmin<LPC>(key);
    const int best = key & 0xffff, minS = key >> 16;
    auto fetch_s = [&](int d) -> int {
        const int j = (d >> 1) % NPL;
        int v;
        if constexpr (NPL == 16) {
            const bool b0 = j & 1, b1 = j & 2, b2 = j & 4;
            const int t0 = b0 ? S[1] : S[0], t1 = b0 ? S[3] : S[2], t2 = b0 ? S[5] : S[4], t3 = b0 ? S[7] : S[6];
            const int t4 = b0 ? S[9] : S[8], t5 = b0 ? S[11] : S[10], t6 = b0 ? S[13] : S[12], t7 = b0 ? S[15] : S[14];
            const int u0 = b1 ? t1 : t0, u1 = b1 ? t3 : t2, u2 = b1 ? t5 : t4, u3 = b1 ? t7 : t6;
            const int w0 = b2 ? u1 : u0, w1 = b2 ? u3 : u2;
            v = (j & 8) ? w1 : w0;
        } else if constexpr (NPL == 8) {
            const int t0 = (j & 1) ? S[1] : S[0], t1 = (j & 1) ? S[3] : S[2], t2 = (j & 1) ? S[5] : S[4], t3 = (j & 1) ? S[7] : S[6];
            const int u0 = (j & 2) ? t1 : t0, u1 = (j & 2) ? t3 : t2;
            v = (j & 4) ? u1 : u0;
        } else {
            const int t0 = (j & 1) ? S[1] : S[0], t1 = (j & 1) ? S[3] : S[2];
            v = (j & 2) ? t1 : t0;
        }
        const int val = (d & 1) ? hi16(v) : lo16(v);
        return grp_allmin<LPC>(((d / (2 * NPL)) == k) ? val : 0x7fffffff);
    };
    const int dm = max(best - 1, 0), dp = min(best + 1, g.D - 1);
    const int sm = fetch_s(dm), sp = fetch_s(dp);
    bool bad = false;
    if (g.uniq > 0) {
        const int T = ceil_div_small(minS * 100, a, inv_a);
        int cnt;
        if (T > 32767) cnt = valid ? 2 * NPL : 0;
        else {
            const int Tpk = pk_dup(max(T, -32768));
            int acc = 0;
#pragma unroll
            for (int j = 0; j < NPL; j++) {
                const int diff = as_i(__builtin_elementwise_sub_sat(as_s(S[j]), as_s(Tpk)));
                acc = pk_sub(acc, as_i(as_s(diff) >> (s16x2){15, 15}));
            }
            cnt = valid ? lo16(acc) + hi16(acc) : 0;
        }
        cnt = grp_allsum<LPC>(cnt);
        int win = (minS < T) ? 1 : 0;
        if (best > 0 && sm < T) win++;
        if (best < g.D - 1 && sp < T) win++;
        bad = cnt > win;
    }
    int dsp = g.invalid;
    if (!bad) {
        dsp = best * 16;
        if (0 < best && best < g.D - 1) {
            const int den = max(sm + sp - 2 * minS, 1);
            dsp += trunc_div_small((sm - sp) * 16 + den, den * 2);
        }
        dsp += g.minD * 16;
    }
    dsp_out = dsp;
    minS_out = minS;
}

// ---------------------------------------------------------------------------------------------------------
// MODE_HH (OpenCV computeDisparitySGBM with fullDP): eight full-length paths over the one-stripe cost volume, folded into
// S = sat16(S + L_r) in the contract order of the directions r = p - q:
//   (+1,0) (+1,+1) (0,+1) (-1,+1)  (pass 1)   (-1,0) (+1,-1) (0,-1) (-1,-1)  (pass 2)
// k_hh_path runs ONE direction over every line of its family (rows, columns, diagonals x-y = c, anti-diagonals x+y = c) with
// the generic lane mapping (a disparity vector on LPC lanes x NPL packed registers, 64/LPC adjacent lines per wave):
// one chain per line, each step moves by the family-constant stride (dy*W1 + dx)*DPW words in the [y][x][dp] volume, and the
// loads of the next HH_RING steps are in flight while a step runs.
// FOLD 0: S = L (first direction); 1: S = sat16(S + L); 2: the same, then wta_regs on the finished S into raw / mins (S is not
// stored).  The lines of one wave may differ in length (diagonals): a lane group past the end of its line keeps stepping on
// its last pixel's loads and stores nothing.
constexpr int HH_RING = 16;
template <int NPL, int LPC, bool PADDED, int FOLD>
__global__ void __launch_bounds__(64) k_hh_path(const int *__restrict__ cvol, int *__restrict__ svol, SgmGeom g, int dx, int dy,
                                                float inv_a, int16_t *__restrict__ raw, int16_t *__restrict__ mins) {
    constexpr int DPW = NPL * LPC, LPW = 64 / LPC;
    static_assert(NPL == 4, "one 16-byte load per lane and volume");
    const int lane = threadIdx.x, k = lane % LPC;
    const int W1 = g.W1, H = g.H;
    const int nlines = dy == 0 ? H : dx == 0 ? W1 : W1 + H - 1;
    const int lraw = blockIdx.x * LPW + lane / LPC;
    const bool line_ok = lraw < nlines;
    const int li = min(lraw, nlines - 1);
    int x0, y0, n;   // first pixel of line li in the direction of travel, and the line's length
    if (dy == 0) {
        y0 = li; x0 = dx > 0 ? 0 : W1 - 1; n = W1;
    } else if (dx == 0) {
        x0 = li; y0 = dy > 0 ? 0 : H - 1; n = H;
    } else if (dx == dy) {                                  // x - y = li - (H - 1); (xs, ys) = the top-left end
        const int c = li - (H - 1), xs = max(c, 0), ys = max(-c, 0);
        n = min(W1 - xs, H - ys);
        x0 = dy > 0 ? xs : xs + n - 1; y0 = dy > 0 ? ys : ys + n - 1;
    } else {                                                // x + y = li; (xs, ys) = the top-right end
        const int ys = max(li - (W1 - 1), 0), xs = li - ys;
        n = min(xs + 1, H - ys);
        x0 = dy > 0 ? xs : xs - (n - 1); y0 = dy > 0 ? ys : ys + n - 1;
    }
    const int nmax = __builtin_amdgcn_readfirstlane(wave_allmax_i32(n));
    const long stride = ((long)dy * W1 + dx) * DPW;
    const long base = ((long)y0 * W1 + x0) * DPW + k * NPL;
    const bool valid = 2 * NPL * k < g.D, first = k == 0, last = k == LPC - 1;
    const int P1pk = pk_dup(g.P1), a = 100 - g.uniq;
    int P[NPL], minp = 0;
#pragma unroll
    for (int j = 0; j < NPL; j++) P[j] = valid ? 0 : PADPK;
    int cb[HH_RING][NPL], sb[HH_RING][NPL];
    auto load = [&](int (&c)[NPL], int (&s)[NPL], int i) {
        const long o = base + (long)min(i, n - 1) * stride;
        const int4 cv = *(const int4 *)(cvol + o);
        c[0] = cv.x; c[1] = cv.y; c[2] = cv.z; c[3] = cv.w;
        if (FOLD > 0) {
            const int4 sv = *(const int4 *)(svol + o);
            s[0] = sv.x; s[1] = sv.y; s[2] = sv.z; s[3] = sv.w;
        }
    };
    auto step = [&](const int (&c)[NPL], const int (&s)[NPL], int i) {
        sgm_step_g<NPL, LPC, PADDED>(P, minp, c, P1pk, g.P2, first, last, valid);
        const bool on = line_ok && i < n;
        int S[NPL];
#pragma unroll
        for (int j = 0; j < NPL; j++) S[j] = FOLD == 0 ? P[j] : pk_add_sat(s[j], P[j]);
        if (FOLD < 2) {
            if (on) *(int4 *)(svol + base + (long)i * stride) = make_int4(S[0], S[1], S[2], S[3]);
        } else {
            int dsp, minS;
            wta_regs<NPL, LPC>(S, k, valid, g, a, inv_a, dsp, minS);
            if (on && first) {
                const size_t q = (size_t)(y0 + i * dy) * g.W + g.minX1 + x0 + i * dx;
                raw[q] = (int16_t)dsp;
                mins[q] = (int16_t)minS;
            }
        }
    };
#pragma unroll
    for (int u = 0; u < HH_RING; u++) load(cb[u], sb[u], u);
#pragma unroll 1
    for (int i0 = 0; i0 < nmax; i0 += HH_RING) {
#pragma unroll
        for (int u = 0; u < HH_RING; u++) {
            step(cb[u], sb[u], i0 + u);
            load(cb[u], sb[u], i0 + u + HH_RING);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------
// k_lrcheck: per row: rebuild OpenCV's disp2 / disp2cost scatter (lowest cost wins, among equal costs the
// LARGEST x, because the original sweeps x right-to-left with a strict '>') with one LDS atomicMin on the key
// (cost+32768)<<16 | (w-1-x), then apply the two-sided disp12MaxDiff test.  Output covers all w columns.
__global__ void __launch_bounds__(256) k_lrcheck(const int16_t *__restrict__ raw, const int16_t *__restrict__ mins, SgmGeom g,
                                                 int16_t *__restrict__ out) {
    extern __shared__ unsigned keys[];
    const int y = blockIdx.x, W = g.W;
    const int16_t *r = raw + (size_t)y * W, *m = mins + (size_t)y * W;
    for (int x = threadIdx.x; x < W; x += 256) keys[x] = 0xffffffffu;
    __syncthreads();
    // four strides of loads in flight per thread (a rolled loop waits for each 2-byte load before the next: 13 dependent round
    // trips per phase at C2's width were most of this kernel's 41 us)
    for (int x0 = g.minX1 + (int)threadIdx.x; x0 < g.maxX1; x0 += 4 * 256) {
        int d1v[4], mv[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int x = min(x0 + 256 * u, g.maxX1 - 1);
            d1v[u] = r[x]; mv[u] = m[x];
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int x = x0 + 256 * u, d1 = d1v[u];
            if (x >= g.maxX1 || d1 == g.invalid) continue;
            const int d = (d1 + 7) >> 4;  // best + minD (sub-pixel offset lies in [-7, 8])
            const int x2 = x - d;
            atomicMin(&keys[x2], ((unsigned)(mv[u] + 32768) << 16) | (unsigned)(W - 1 - x));
        }
    }
    __syncthreads();
    int d1n[4];
#pragma unroll
    for (int u = 0; u < 4; u++) d1n[u] = r[min((int)threadIdx.x + 256 * u, W - 1)];
    for (int xb = (int)threadIdx.x; xb < W; xb += 4 * 256) {
        int d1c[4];
#pragma unroll
        for (int u = 0; u < 4; u++) { d1c[u] = d1n[u]; d1n[u] = r[min(xb + 4 * 256 + 256 * u, W - 1)]; }
#pragma unroll
        for (int u = 0; u < 4; u++) {
        const int x = xb + 256 * u;
        if (x >= W) continue;
        int d1 = g.invalid;
        if (x >= g.minX1 && x < g.maxX1) {
            d1 = d1c[u];
            if (d1 != g.invalid) {
                const int _d = d1 >> 4, d_ = (d1 + 15) >> 4;
                const int _x = x - _d, x_ = x - d_;
                // QUIRK: an unset disp2 entry holds the SCALED invalid marker (minD-1)*16, which passes the ">= minD"
                // test whenever minD >= 2 and then counts as a disagreeing match
                bool f1 = false, f2 = false;
                if (0 <= _x && _x < W) {
                    const int d2 = keys[_x] != 0xffffffffu ? (W - 1 - (int)(keys[_x] & 0xffffu)) - _x : g.invalid;
                    f1 = d2 >= g.minD && abs(d2 - _d) > g.d12;
                }
                if (0 <= x_ && x_ < W) {
                    const int d2 = keys[x_] != 0xffffffffu ? (W - 1 - (int)(keys[x_] & 0xffffu)) - x_ : g.invalid;
                    f2 = d2 >= g.minD && abs(d2 - d_) > g.d12;
                }
                if (f1 && f2) d1 = g.invalid;
            }
        }
        out[(size_t)y * W + x] = (int16_t)d1;
        }
    }
}

// QUIRK_SMALL_IMAGE_STRIPES (oracle/sgbm3way.c has the derivation): on images so small that a stripe's warm-up start is clamped to
// row 0 (stripe_sz < overlap: H <= 12 at blockSize 5) the original assembles that stripe's rows from the wrong rows of its private
// buffer: out[n * stripe_sz + j] = row overlap + j of a run that started at row 0, and rows the run never wrote are uninitialised
// memory there (the invalid marker here).  `run0` is the LR-checked map of ONE run over the whole image from row 0.
__global__ void __launch_bounds__(256) k_tiny_assemble(int16_t *__restrict__ lrd, const int16_t *__restrict__ run0, SgmGeom g) {
    const int x = blockIdx.x * 256 + threadIdx.x, i = blockIdx.y;
    if (x >= g.W) return;
    const int n = i / g.stripe_sz;
    if (n < 1 || n * g.stripe_sz - g.overlap >= 0) return;
    const int r = g.overlap + (i - n * g.stripe_sz), src_end = min((n + 1) * g.stripe_sz, g.H);
    lrd[(size_t)i * g.W + x] = r < src_end ? run0[(size_t)r * g.W + x] : (int16_t)g.invalid;
}

// k_median3: medianBlur(disp, 3) on int16 with replicated borders
__device__ __forceinline__ void cswap(int &a, int &b) { int lo = min(a, b), hi = max(a, b); a = lo; b = hi; }
__global__ void __launch_bounds__(256) k_median3(const int16_t *__restrict__ src, int16_t *__restrict__ dst, int W, int H) {
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= W) return;
    const int16_t *r0 = src + (size_t)max(y - 1, 0) * W, *r1 = src + (size_t)y * W, *r2 = src + (size_t)min(y + 1, H - 1) * W;
    const int xl = max(x - 1, 0), xr = min(x + 1, W - 1);
    int p0 = r0[xl], p1 = r0[x], p2 = r0[xr], p3 = r1[xl], p4 = r1[x], p5 = r1[xr], p6 = r2[xl], p7 = r2[x], p8 = r2[xr];
    cswap(p1, p2); cswap(p4, p5); cswap(p7, p8); cswap(p0, p1); cswap(p3, p4); cswap(p6, p7);
    cswap(p1, p2); cswap(p4, p5); cswap(p7, p8); cswap(p0, p3); cswap(p5, p8); cswap(p4, p7);
    cswap(p3, p6); cswap(p1, p4); cswap(p2, p5); cswap(p4, p7); cswap(p4, p2); cswap(p6, p4);
    cswap(p4, p2);
    dst[(size_t)y * W + x] = (int16_t)p4;
}

// ---------------------------------------------------------------------------------------------------------
// filterSpeckles(disp, newVal, maxSpeckleSize, maxDiff) (called by StereoSGBM.compute iff speckleWindowSize > 0, the
// depth4.py / depth_test.py parameter family): 4-connected components of pixels != newVal whose neighbouring values
// differ by <= maxDiff; components of at most maxSpeckleSize pixels are set to newVal.  The original flood-fills in
// raster order; component membership does not depend on the order, so a lock-free union-find gives the same image.
__device__ __forceinline__ int uf_find(int *L, int i) {
    int p = __hip_atomic_load(&L[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    while (p != i) { i = p; p = __hip_atomic_load(&L[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    return i;
}
__device__ __forceinline__ void uf_union(int *L, int a, int b) {
    for (;;) {
        a = uf_find(L, a);
        b = uf_find(L, b);
        if (a == b) return;
        if (a < b) { int t = a; a = b; b = t; }   // link the larger root to the smaller one
        const int old = atomicMin(&L[a], b);
        if (old == a) return;
        a = old;
    }
}
__global__ void __launch_bounds__(256) k_spk_init(const int16_t *__restrict__ img, int n, int newVal, int *__restrict__ L, int *__restrict__ cnt) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    L[i] = img[i] != newVal ? i : -1;
    cnt[i] = 0;
}
__global__ void __launch_bounds__(256) k_spk_merge(const int16_t *__restrict__ img, int W, int H, int newVal, int maxDiff, int *__restrict__ L) {
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= W) return;
    const int i = y * W + x, v = img[i];
    if (v == newVal) return;
    if (x + 1 < W) { const int u = img[i + 1]; if (u != newVal && abs(v - u) <= maxDiff) uf_union(L, i, i + 1); }
    if (y + 1 < H) { const int u = img[i + W]; if (u != newVal && abs(v - u) <= maxDiff) uf_union(L, i, i + W); }
}
__global__ void __launch_bounds__(256) k_spk_count(int n, int *__restrict__ L, int *__restrict__ cnt) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n || L[i] < 0) return;
    const int r = uf_find(L, i);
    L[i] = r;                       // flatten (every thread only shortens its own entry)
    atomicAdd(&cnt[r], 1);
}
__global__ void __launch_bounds__(256) k_spk_apply(int16_t *__restrict__ img, int n, int newVal, int maxSize, const int *__restrict__ L,
                                                   const int *__restrict__ cnt) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int r = L[i];
    if (r >= 0 && cnt[r] <= maxSize) img[i] = (int16_t)newVal;
}

// ---------------------------------------------------------------------------------------------------------
// k_selftest: checks the cross-lane building blocks against their definition.
__global__ void __launch_bounds__(64) k_selftest(int *out) {
    const int lane = threadIdx.x;
    int bad = 0;
    const int v = (lane * 37 + 11) % 101 - 50;
    if (wave_shr1(v, -777) != (lane == 0 ? -777 : ((lane - 1) * 37 + 11) % 101 - 50)) bad |= 1;
    if (wave_shl1(v, -777) != (lane == 63 ? -777 : ((lane + 1) * 37 + 11) % 101 - 50)) bad |= 2;
    int mn = 1 << 30, mx = -(1 << 30);
    for (int l = 0; l < 64; l++) { int t = (l * 37 + 11) % 101 - 50; mn = min(mn, t); mx = max(mx, t); }
    if (wave_allmin_i32(v) != mn) bad |= 4;
    if (wave_allmax_i32(v) != mx) bad |= 8;
    {
        int first = 0;  // first lane holding the minimum: the WTA key relies on "smallest index wins among ties"
        for (int l = 63; l >= 0; l--) if ((l * 37 + 11) % 101 - 50 == mn) first = l;
        if (wave_allmin_u32((unsigned)(v + 100) << 8 | (unsigned)lane) != (((unsigned)(mn + 100) << 8) | (unsigned)first)) bad |= 16;
    }
    // packed helpers
    if (pk_add_sat(0x7fff7fff, pk_dup(600)) != 0x7fff7fff) bad |= 32;
    if (pk_min(0x00050003, (int)0xfffe0004) != (int)0xfffe0003) bad |= 64;
    if (pk_usub_sat(0x00050003, 0x00070001) != 0x00000002) bad |= 128;
    if (__builtin_amdgcn_alignbit(0x11112222, 0x33334444, 16) != 0x22223333) bad |= 256;
    if (__builtin_amdgcn_perm(0xa3a2a1a0u, 0xb3b2b1b0u, 0x0c050c01) != 0x00a100b1u) bad |= 512;
    // one sgm_step against the scalar definition, D = 128
    {
        int P[1] = {(((lane * 7) % 13) & 0xffff) | ((((lane * 5) % 11)) << 16)};
        int minp = 0;
        int allmin = wave_allmin_i32(min(lo16(P[0]), hi16(P[0])));
        minp = allmin;
        const int C[1] = {((lane + 3) & 0xffff) | ((2 * lane + 1) << 16)};
        const int P1 = 3, P2 = 9;
        // scalar reference for this lane's two disparities
        auto Lp = [&](int d) -> int { if (d < 0 || d > 127) return 32767; int l = d >> 1; return (d & 1) ? (l * 5) % 11 : (l * 7) % 13; };
        int want[2];
        for (int h = 0; h < 2; h++) {
            int d = 2 * lane + h;
            int m = min(min(Lp(d), minp + P2), min(Lp(d - 1), Lp(d + 1)) + P1);
            int c = h ? 2 * lane + 1 : lane + 3;
            want[h] = c + m - (minp + P2);
        }
        sgm_step<1>(P, minp, C, pk_dup(P1), P2, true);
        if (lo16(P[0]) != want[0] || hi16(P[0]) != want[1]) bad |= 1024;
        int wm = wave_allmin_i32(min(want[0], want[1]));
        if (minp != wm) bad |= 2048;
    }
    // dual-chain step == two single steps
    {
        int PA[1] = {(((lane * 7) % 13) & 0xffff) | ((((lane * 5) % 11)) << 16)}, PB[1] = {(((lane * 3) % 17) & 0xffff) | ((((lane * 11) % 7)) << 16)};
        int mA = wave_allmin_i32(min(lo16(PA[0]), hi16(PA[0]))), mB = wave_allmin_i32(min(lo16(PB[0]), hi16(PB[0])));
        const int CA[1] = {((lane + 3) & 0xffff) | ((2 * lane + 1) << 16)}, CB[1] = {((5 * lane + 2) & 0xffff) | ((lane + 9) << 16)};
        int dA = PA[0], dB = PB[0], mAB = (mA & 0xffff) | (mB << 16);
        for (int it = 0; it < 3; it++) {
            sgm_step_g<1, 64, false>(PA, mA, CA, pk_dup(3), 9, lane == 0, lane == 63, true);
            sgm_step_g<1, 64, false>(PB, mB, CB, pk_dup(3), 9, lane == 0, lane == 63, true);
            sgm_step_dual<false>(dA, dB, mAB, CA[0], CB[0], pk_dup(3), pk_dup(9), true);
            if (dA != PA[0] || dB != PB[0] || lo16(mAB) != mA || hi16(mAB) != mB) bad |= 1 << 23;
        }
    }
    // generic dual step (2 registers x 32 lanes) == two generic single steps
    {
        const int kk = lane % 32;
        int PA[2] = {(((lane * 7) % 13) & 0xffff) | ((((lane * 5) % 11)) << 16), ((lane * 3) % 19) | (((lane + 4) % 23) << 16)};
        int PB[2] = {(((lane * 3) % 17) & 0xffff) | ((((lane * 11) % 7)) << 16), ((lane * 9) % 29) | (((lane * 2 + 1) % 31) << 16)};
        int mA = grp_allmin<32>(min(min(lo16(PA[0]), hi16(PA[0])), min(lo16(PA[1]), hi16(PA[1]))));
        int mB = grp_allmin<32>(min(min(lo16(PB[0]), hi16(PB[0])), min(lo16(PB[1]), hi16(PB[1]))));
        const int CA[2] = {((lane + 3) & 0xffff) | ((2 * lane + 1) << 16), (lane % 7) | ((lane % 5) << 16)};
        const int CB[2] = {((5 * lane + 2) & 0xffff) | ((lane + 9) << 16), (lane % 3) | ((lane % 11) << 16)};
        int dA[2] = {PA[0], PA[1]}, dB[2] = {PB[0], PB[1]}, mAB = (mA & 0xffff) | (mB << 16);
        for (int it = 0; it < 3; it++) {
            sgm_step_g<2, 32, false>(PA, mA, CA, pk_dup(3), 9, kk == 0, kk == 31, true);
            sgm_step_g<2, 32, false>(PB, mB, CB, pk_dup(3), 9, kk == 0, kk == 31, true);
            sgm_step_dual_g<2, 32, false>(dA, dB, mAB, CA, CB, pk_dup(3), pk_dup(9), kk == 0, kk == 31, true);
            if (dA[0] != PA[0] || dA[1] != PA[1] || dB[0] != PB[0] || dB[1] != PB[1] || lo16(mAB) != mA || hi16(mAB) != mB) bad |= 1 << 24;
        }
        // and the 2x32 single step against the scalar definition
        int Q[2] = {(((lane * 7) % 13) & 0xffff) | ((((lane * 5) % 11)) << 16), ((lane * 3) % 19) | (((lane + 4) % 23) << 16)};
        auto Lp = [&](int grp, int d) -> int {
            if (d < 0 || d > 127) return 32767;
            const int l = grp * 32 + d / 4, r = (d / 2) % 2, hh = d % 2;
            const int v0 = (((l * 7) % 13) & 0xffff) | ((((l * 5) % 11)) << 16), v1 = ((l * 3) % 19) | (((l + 4) % 23) << 16);
            const int v = r ? v1 : v0;
            return hh ? hi16(v) : lo16(v);
        };
        int mq = grp_allmin<32>(min(min(lo16(Q[0]), hi16(Q[0])), min(lo16(Q[1]), hi16(Q[1]))));
        const int mq0 = mq;
        sgm_step_g<2, 32, false>(Q, mq, CA, pk_dup(3), 9, kk == 0, kk == 31, true);
        for (int r = 0; r < 2; r++)
            for (int hh = 0; hh < 2; hh++) {
                const int d = 4 * kk + 2 * r + hh, grp = lane / 32;
                const int mm = min(min(Lp(grp, d), mq0 + 9), min(Lp(grp, d - 1), Lp(grp, d + 1)) + 3);
                const int c = hh ? hi16(CA[r]) : lo16(CA[r]);
                const int got = hh ? hi16(Q[r]) : lo16(Q[r]);
                if (got != c + mm - (mq0 + 9)) bad |= 1 << 25;
            }
    }
    // generic group helpers, LPC = 8 and 16
    {
        auto val = [](int l) { return (l * 37 + 11) % 101 - 50; };
        const int k8 = lane % 8, k16 = lane % 16;
        if (grp_shr1<8>(v, -777, k8 == 0) != (k8 == 0 ? -777 : val(lane - 1))) bad |= 1 << 12;
        if (grp_shl1<8>(v, -777, k8 == 7) != (k8 == 7 ? -777 : val(lane + 1))) bad |= 1 << 13;
        if (grp_shr1<16>(v, -777, k16 == 0) != (k16 == 0 ? -777 : val(lane - 1))) bad |= 1 << 14;
        if (grp_shl1<16>(v, -777, k16 == 15) != (k16 == 15 ? -777 : val(lane + 1))) bad |= 1 << 15;
        int m8 = 1 << 30, s8 = 0, m16 = 1 << 30, s16 = 0;
        for (int l = lane - k8; l < lane - k8 + 8; l++) { m8 = min(m8, val(l)); s8 += val(l); }
        for (int l = lane - k16; l < lane - k16 + 16; l++) { m16 = min(m16, val(l)); s16 += val(l); }
        if (grp_allmin<8>(v) != m8) bad |= 1 << 16;
        if (grp_allsum<8>(v) != s8) bad |= 1 << 17;
        if (grp_allmin<16>(v) != m16) bad |= 1 << 18;
        if (grp_allsum<16>(v) != s16) bad |= 1 << 19;
        if (grp_allmin<64>(v) != mn) bad |= 1 << 20;
        // exact small divisions
        const int nn = (lane - 31) * 4099 + 7, dd = 2 * (lane * 37 + 1);
        if (trunc_div_small(nn, dd) != nn / dd) bad |= 1 << 21;
        const int thr = (lane - 20) * 997 * 100, aa = 85;
        int T = ceil_div_small(thr, aa, 1.0f / 85.0f);
        if (!(T * aa >= thr && (T - 1) * aa < thr)) bad |= 1 << 22;
    }
    atomicOr(out, bad);
}

// ---------------------------------------------------------------------------------------------------------
// k_streambench (diagnostic, not on the product path): every wave streams through its own `row_bytes`-long row,
// MODE 0: 4 B/lane requests (256 B per wave-instruction, the access shape of k_hscan), MODE 1: 16 B/lane (1 KB);
// `write` adds a store of the same shape to a second buffer.  Used to price access shapes.
template <int MODE, int NTL, int NTS>
__global__ void __launch_bounds__(64) k_streambench(const int *__restrict__ in, int *__restrict__ out, size_t row_words, int write, int delay) {
    const int lane = threadIdx.x;
    const int *r = in + (size_t)blockIdx.x * row_words;
    int *o = out + (size_t)blockIdx.x * row_words;
    int acc = 0;
    if (MODE == 0) {
        for (size_t x = 0; x + 64 * 16 <= row_words; x += 64 * 16) {
            int v[16];
#pragma unroll
            for (int u = 0; u < 16; u++) v[u] = NTL ? __builtin_nontemporal_load(&r[x + u * 64 + lane]) : r[x + u * 64 + lane];
#pragma unroll
            for (int u = 0; u < 16; u++) {
                acc += v[u];
                for (int d = 0; d < delay; d++) acc = __builtin_amdgcn_update_dpp(acc, acc, 0xB1, 0xf, 0xf, false) + 1;
                if (write) {
                    if (NTS) __builtin_nontemporal_store(acc, &o[x + u * 64 + lane]);
                    else o[x + u * 64 + lane] = acc;
                }
            }
        }
    } else {
        typedef int v4i __attribute__((ext_vector_type(4)));
        for (size_t x = 0; x + 256 * 4 <= row_words; x += 256 * 4) {
            v4i v[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const v4i *q = (const v4i *)&r[x + u * 256 + lane * 4];
                v[u] = NTL ? __builtin_nontemporal_load(q) : *q;
            }
#pragma unroll
            for (int u = 0; u < 4; u++) {
                acc += v[u].x + v[u].y + v[u].z + v[u].w;
                for (int d = 0; d < 4 * delay; d++) acc = __builtin_amdgcn_update_dpp(acc, acc, 0xB1, 0xf, 0xf, false) + 1;
                if (write) {
                    const v4i w4 = {acc, acc, acc, acc};
                    v4i *q = (v4i *)&o[x + u * 256 + lane * 4];
                    if (NTS) __builtin_nontemporal_store(w4, q);
                    else *q = w4;
                }
            }
        }
    }
    if (acc == 0x12345678) out[0] = acc;
}

// worst-case block cost of a pair (all CN channels summed) above 16383: the cost kernel then tracks the actual maximum
inline bool sgm_track(const SgmGeom &g) { return (long)g.CN * (2 * g.SH2 + 1) * (2 * g.SH2 + 1) * (2L * g.ftzero + 63) > 16383; }

int derive_geom(r3d_ctx *ctx, const r3d_sgbm_params *p, int w, int h, int cn, SgmGeom &g) {
    if (!p) return r3d_fail(ctx, R3D_E_BADARG, "sgbm: params is NULL");
    if (cn != 1 && cn != 3) return r3d_fail(ctx, R3D_E_BADARG, "sgbm: images must have 1 or 3 channels, got %d", cn);
    g.CN = cn;
    if (p->mode != R3D_SGBM_MODE_3WAY && p->mode != R3D_SGBM_MODE_HH)
        return r3d_fail(ctx, R3D_E_UNSUPPORTED,
                        "sgbm: only mode=STEREO_SGBM_MODE_HH (1) and STEREO_SGBM_MODE_SGBM_3WAY (2) are implemented, got %d", p->mode);
    if (p->numDisparities <= 0 || p->numDisparities % 16 != 0)
        return r3d_fail(ctx, R3D_E_BADARG, "sgbm: numDisparities must be a positive multiple of 16, got %d", p->numDisparities);
    if (p->numDisparities > 512) return r3d_fail(ctx, R3D_E_UNSUPPORTED, "sgbm: numDisparities > 512 not supported (got %d)", p->numDisparities);
    if (p->blockSize < 1 || p->blockSize % 2 == 0 || p->blockSize > 11)
        return r3d_fail(ctx, R3D_E_BADARG, "sgbm: blockSize must be odd in [1, 11], got %d", p->blockSize);
    if (w <= 0 || h <= 0 || w > 65536) return r3d_fail(ctx, R3D_E_BADARG, "sgbm: bad image size %dx%d", w, h);
    g.W = w; g.H = h;
    g.minD = p->minDisparity; g.D = p->numDisparities;
    g.NP = g.D <= 128 ? 1 : 2;   // read by nothing (every kernel and launcher goes by DP); the field stays so that SgmGeom, which every
                                 // kernel takes by value, keeps its argument layout
    g.DP = g.D <= 32 ? 32 : g.D <= 64 ? 64 : g.D <= 128 ? 128 : g.D <= 256 ? 256 : 512;
    const int maxD = g.minD + g.D;
    g.minX1 = maxD > 0 ? maxD : 0;
    g.maxX1 = w + (g.minD < 0 ? g.minD : 0);
    g.W1 = g.maxX1 - g.minX1;
    // W1 <= 0 (the disparity range leaves no column to match) is not an error: the caller fills the map with the invalid marker
    g.SW2 = g.SH2 = p->blockSize / 2;
    g.P1 = p->P1 > 0 ? p->P1 : 2;
    g.P2 = p->P2 > 0 ? p->P2 : 5;
    if (g.P2 < g.P1 + 1) g.P2 = g.P1 + 1;
    g.uniq = p->uniquenessRatio >= 0 ? p->uniquenessRatio : 10;
    if (g.uniq >= 100) return r3d_fail(ctx, R3D_E_UNSUPPORTED, "sgbm: uniquenessRatio >= 100 not supported (got %d)", g.uniq);
    g.d12 = p->disp12MaxDiff > 0 ? p->disp12MaxDiff : 1;
    g.ftzero = (p->preFilterCap > 15 ? p->preFilterCap : 15) | 1;
    g.stripe_sz = (h + 3) / 4;
    g.overlap = (p->blockSize / 2 + 1) + (g.stripe_sz + 9) / 10;
    g.invalid = (g.minD - 1) * 16;
    // Volume addressing (a DP = 512 volume passes 4 GiB at 8 MP): every row, column-segment and line offset into cost / cspec /
    // hsum / ckpt is formed in size_t or long in every kernel; the only int-typed word products are offsets INSIDE one row
    // (x * DP/2 <= 65536 * 256 = 2^24 by the width check above) and LDS indices, so no further argument check is needed.
    // exact-int16 envelope (DESIGN.md "arithmetic envelope"): no packed add may wrap
    // static half: the block cost must fit int16 at all and P2 <= 16383; when the worst-case block cost exceeds 16383
    // the cost kernel tracks the actual maximum and the call fails loudly only if THIS image pair leaves the envelope
    // (a colour pair's block cost is the sum over its channels, so the bound carries the channel count)
    const long cmax = (long)cn * p->blockSize * p->blockSize * (2L * g.ftzero + 63);
    if (cmax > 32767 || g.P2 > 16383 || g.ftzero > 127)
        return r3d_fail(ctx, R3D_E_UNSUPPORTED,
                        "sgbm: blockSize=%d preFilterCap=%d P2=%d channels=%d leave the exact int16 envelope (max block cost %ld > 32767 or P2 > 16383)",
                        p->blockSize, p->preFilterCap, g.P2, cn, cmax);
    if ((long)g.minD * 16 - 16 < -32768 || ((long)maxD) * 16 > 32767)
        return r3d_fail(ctx, R3D_E_BADARG, "sgbm: disparity range [%d, %d) does not fit the x16 int16 output", g.minD, maxD);
    return R3D_OK;
}

// One launch of k_cost2: the block cost of channel `chan` (its record planes), stored (ACC false: channel 0) or added to what the
// earlier channels stored (ACC: chan > 0; see k_cost2), for the main volume and the stripe-top rows alike.
template <int LPC, int SH2, bool TRACK, bool ACC>
int launch_cost2_n(r3d_ctx *ctx, r3d_sgm_ws &ws, const SgmGeom &g, hipStream_t st, int chan) {
    constexpr int NWAVE = 8, CW = 64 / LPC, TC = NWAVE * CW, TO = TC - 2 * SH2;   // 8 waves: 64-column tiles at 128 slots, 2*SH2 of them halo
    static_assert(TO > 0, "tile too small for this block size");
    const int tiles = (g.W1 + TO - 1) / TO;
    // size the row bands so that one round of workgroups fills the chip (each band pays 2*SH2 extra rows of pixel cost)
    // occupancy x CU count, queried once per instantiation AND device (contexts of different devices / threads may race here: the
    // slot is written once with a complete value, readers see 0 or that value)
    static std::atomic<int> slots_of[R3D_MAX_DEVICES];
    const int dev = ctx->device >= 0 && ctx->device < R3D_MAX_DEVICES ? ctx->device : 0;
    int slots = slots_of[dev].load(std::memory_order_relaxed);
    if (slots == 0) {
        int v = 1, c = 256;
        (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&v, (const void *)k_cost2<LPC, SH2, TRACK, NWAVE, ACC>, NWAVE * 64, 0);
        (void)hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, ctx->device);
        slots = (v < 1 ? 1 : v) * (c < 1 ? 256 : c);
        slots_of[dev].store(slots, std::memory_order_relaxed);
    }
    int nb = slots / tiles;
    if (nb < 1) nb = 1;
    int BAND = (g.H + nb - 1) / nb;
    if (BAND < 16) BAND = 16;
    const int nMain = (g.H + BAND - 1) / BAND;
    const int nSpec = SH2 > 0 ? 3 : 0;
    int *maxc = (int *)ws.flags.p + 8;
    if (TRACK) R3D_HIP(ctx, hipMemsetAsync(maxc, 0, 4, st));
    const size_t plane = (size_t)chan * g.W * g.H;
    k_cost2<LPC, SH2, TRACK, NWAVE, ACC><<<dim3(tiles, nMain + nSpec), NWAVE * 64, 0, st>>>(
        (const uint2 *)ws.rec_l.p + plane, (const uint2 *)ws.rec_r.p + plane, g, (int *)ws.cost.p, (int *)ws.cspec.p, BAND, nMain, maxc, 0);
    R3D_HIP(ctx, hipGetLastError());
    if (TRACK) {
        // data-dependent half of the exact-int16 envelope: only reached when the static bound cannot prove it
        int m = 0;
        R3D_HIP(ctx, hipMemcpyAsync(&m, maxc, 4, hipMemcpyDeviceToHost, st));
        R3D_HIP(ctx, hipStreamSynchronize(st));
        if (m > 16383)
            return r3d_fail(ctx, R3D_E_UNSUPPORTED, "sgbm: block cost reaches %d > 16383 on this image pair; outside the exact int16 envelope", m);
    }
    return R3D_OK;
}
template <int LPC, bool ACC>
int launch_cost2_l(r3d_ctx *ctx, r3d_sgm_ws &ws, const SgmGeom &g, hipStream_t st, int chan) {
    const bool track = sgm_track(g) && chan == g.CN - 1;   // on the summed value: the last channel's launch
#define R3D_C2(S, T) launch_cost2_n<LPC, S, T, ACC>(ctx, ws, g, st, chan)
    switch (g.SH2) {
        case 0: return R3D_C2(0, false);
        case 1: return R3D_C2(1, false);
        case 2: return R3D_C2(2, false);
        case 3: return track ? R3D_C2(3, true) : R3D_C2(3, false);
        case 4: return track ? R3D_C2(4, true) : R3D_C2(4, false);
        default:   // blockSize 11: always tracked; three channels of it never pass the static bound of derive_geom
            if constexpr (ACC) return r3d_fail(ctx, R3D_E_UNSUPPORTED, "sgbm: blockSize 11 with 3-channel images is outside the exact int16 envelope");
            else return R3D_C2(5, true);
    }
#undef R3D_C2
}
// the whole cost stage of a pair: channel 0 stores C, the further channels of a colour pair add theirs (cost and cspec alike)
int launch_cost2(r3d_ctx *ctx, r3d_sgm_ws &ws, const SgmGeom &g, hipStream_t st) {
    for (int chan = 0; chan < g.CN; chan++) {
        int rc;
#define R3D_CL(LPC) rc = chan > 0 ? launch_cost2_l<LPC, true>(ctx, ws, g, st, chan) : launch_cost2_l<LPC, false>(ctx, ws, g, st, chan)
        switch (g.DP) {  // LPC = DP / 16 lanes per column
            case 32: R3D_CL(2); break;
            case 64: R3D_CL(4); break;
            case 128: R3D_CL(8); break;
            case 256: R3D_CL(16); break;
            default: R3D_CL(32); break;   // 512 slots: 2 columns per wave, 16-column tiles
        }
#undef R3D_CL
        if (rc) return rc;
    }
    return R3D_OK;
}
// prefilter of both images, every channel: record planes rec_l / rec_r [CN][h][w]
void launch_prefilter(hipStream_t st, const r3d_sgm_ws &ws, const SgmGeom &g, const uint8_t *d_left, const uint8_t *d_right, int stride) {
    const dim3 grid((g.W + 255) / 256, (g.H + PF_ROWS - 1) / PF_ROWS, 2 * g.CN);
    if (g.CN == 1) k_prefilter<1><<<grid, 256, 0, st>>>(d_left, d_right, stride, g.W, g.H, g.ftzero, (uint2 *)ws.rec_l.p, (uint2 *)ws.rec_r.p);
    else k_prefilter<3><<<grid, 256, 0, st>>>(d_left, d_right, stride, g.W, g.H, g.ftzero, (uint2 *)ws.rec_l.p, (uint2 *)ws.rec_r.p);
}

// launcher of k_hscan2: per slot layout the lane mapping (NPL packed registers x LPC lanes per row, 64 / LPC rows per wave) and the
// segment length K:
//   32 / 64 / 128 slots: 16 lanes per row = 4 rows per wave (612 waves at 2448 rows <= 1024 SIMDs, so no SIMD carries two; with 2 rows
//                        per wave 1224 waves left 200 SIMDs with double work) and 1 / 2 / 4 registers per lane, K = 32 / 16 / 16;
//   256 slots: 4 registers x 32 lanes, 2 rows per wave, K = 6;   512 slots: 4 x 64, ONE row per wave (one more butterfly stage per
//              step), K = 6 as at 256: the same 6 * K * 4 registers of cost / L_left buffers per lane.
// Reserves the checkpoints: one per image row and segment (k_hscan2 addresses them by row), rounded up to whole waves.
template <int NPL, int LPC, int K>
int launch_hscan2_l(r3d_ctx *ctx, r3d_sgm_ws &ws, hipStream_t st, const SgmGeom &g) {
    constexpr int RPW = 64 / LPC, DPW = NPL * LPC;
    const int nwaves = (g.H + RPW - 1) / RPW;
    if (int rc = r3d_reserve(ctx, ws.ckpt, (size_t)(g.H + 8) * (g.W1 / K + 1) * (DPW + 4) * 4)) return rc;
    const int *cp = (const int *)ws.cost.p;
    int *hp = (int *)ws.hsum.p, *kp = (int *)ws.ckpt.p;
    if (g.D != g.DP) k_hscan2<NPL, LPC, K, true><<<nwaves, 64, 0, st>>>(cp, hp, kp, g);
    else k_hscan2<NPL, LPC, K, false><<<nwaves, 64, 0, st>>>(cp, hp, kp, g);
    R3D_HIP(ctx, hipGetLastError());
    return R3D_OK;
}
int launch_hscan2(r3d_ctx *ctx, r3d_sgm_ws &ws, hipStream_t st, const SgmGeom &g) {
    switch (g.DP) {
        case 32: return launch_hscan2_l<1, 16, 32>(ctx, ws, st, g);
        case 64: return launch_hscan2_l<2, 16, 16>(ctx, ws, st, g);
        case 128: return launch_hscan2_l<4, 16, 16>(ctx, ws, st, g);
        case 256: return launch_hscan2_l<4, 32, 6>(ctx, ws, st, g);
        default: return launch_hscan2_l<4, 64, 6>(ctx, ws, st, g);
    }
}

// launcher of k_vscan2, one mapping per slot layout.  128 slots: 16 columns per wave (NPL = 16, LPC = 4: 784 waves at 3136 cost
// columns, no SIMD carries two) where D fills whole 32-disparity lanes, 8 columns (NPL = 8, LPC = 8) otherwise, as at D = 80 or 112.
// 512 slots: 16 disparities per lane on 32 lanes, 2 columns per wave (NPL = 16 would need whole 32-disparity lanes; D is a
// multiple of 16).
void launch_vscan2(hipStream_t st, const SgmGeom &g, float inv_a, const int *cost, const int *cspec, const int *hsum, int16_t *raw, int16_t *mins) {
    if (g.DP == 32) k_vscan2<4, 4><<<dim3((g.W1 + 15) / 16, 4), 64, 0, st>>>(cost, cspec, hsum, g, inv_a, raw, mins, 0);
    else if (g.DP == 64) k_vscan2<8, 4><<<dim3((g.W1 + 15) / 16, 4), 64, 0, st>>>(cost, cspec, hsum, g, inv_a, raw, mins, 0);
    else if (g.DP == 128 && g.D % 32 == 0) k_vscan2<16, 4><<<dim3((g.W1 + 15) / 16, 4), 64, 0, st>>>(cost, cspec, hsum, g, inv_a, raw, mins, 0);
    else if (g.DP == 128) k_vscan2<8, 8><<<dim3((g.W1 + 7) / 8, 4), 64, 0, st>>>(cost, cspec, hsum, g, inv_a, raw, mins, 0);
    else if (g.DP == 256) k_vscan2<8, 16><<<dim3((g.W1 + 3) / 4, 4), 64, 0, st>>>(cost, cspec, hsum, g, inv_a, raw, mins, 0);
    else k_vscan2<8, 32><<<dim3((g.W1 + 1) / 2, 4), 64, 0, st>>>(cost, cspec, hsum, g, inv_a, raw, mins, 0);
}

// MODE_HH directions r = p - q in the order they enter S (pass 1, then pass 2), and their profiling names
constexpr int HH_DIRS[8][2] = {{1, 0}, {1, 1}, {0, 1}, {-1, 1}, {-1, 0}, {1, -1}, {0, -1}, {-1, -1}};
constexpr const char *HH_NAMES[8] = {"hh_right", "hh_down_right", "hh_down", "hh_down_left", "hh_left", "hh_up_right", "hh_up", "hh_up_left_wta"};

// one k_hh_path launch: direction `r` of HH_DIRS; the first direction writes S, the last one selects from it (store_last: it
// stores S like the six before it and touches neither raw nor mins -- r3d_sgm_hh_partial).  LPC = DP / 8 lanes per disparity
// vector (4 packed registers each), 64 / LPC lines per wave.
template <int LPC, bool PADDED>
void launch_hh_path_l(hipStream_t st, const SgmGeom &g, int r, const int *cost, int *svol, float inv_a, int16_t *raw, int16_t *mins, bool store_last) {
    const int dx = HH_DIRS[r][0], dy = HH_DIRS[r][1];
    const int nlines = dy == 0 ? g.H : dx == 0 ? g.W1 : g.W1 + g.H - 1;
    const dim3 grid((nlines + 64 / LPC - 1) / (64 / LPC));
    if (r == 0) k_hh_path<4, LPC, PADDED, 0><<<grid, 64, 0, st>>>(cost, svol, g, dx, dy, inv_a, raw, mins);
    else if (r == 7 && !store_last) k_hh_path<4, LPC, PADDED, 2><<<grid, 64, 0, st>>>(cost, svol, g, dx, dy, inv_a, raw, mins);
    else k_hh_path<4, LPC, PADDED, 1><<<grid, 64, 0, st>>>(cost, svol, g, dx, dy, inv_a, raw, mins);
}
template <int LPC>
void launch_hh_path_p(hipStream_t st, const SgmGeom &g, int r, const int *cost, int *svol, float inv_a, int16_t *raw, int16_t *mins, bool store_last) {
    if (g.D != g.DP) launch_hh_path_l<LPC, true>(st, g, r, cost, svol, inv_a, raw, mins, store_last);
    else launch_hh_path_l<LPC, false>(st, g, r, cost, svol, inv_a, raw, mins, store_last);
}
void launch_hh_path(hipStream_t st, const SgmGeom &g, int r, const int *cost, int *svol, float inv_a, int16_t *raw, int16_t *mins, bool store_last = false) {
    switch (g.DP) {
        case 32: launch_hh_path_p<4>(st, g, r, cost, svol, inv_a, raw, mins, store_last); break;
        case 64: launch_hh_path_p<8>(st, g, r, cost, svol, inv_a, raw, mins, store_last); break;
        case 128: launch_hh_path_p<16>(st, g, r, cost, svol, inv_a, raw, mins, store_last); break;
        case 512: launch_hh_path_p<64>(st, g, r, cost, svol, inv_a, raw, mins, store_last); break;   // one line per wave
        default: launch_hh_path_p<32>(st, g, r, cost, svol, inv_a, raw, mins, store_last); break;
    }
}

}  // namespace

// MODE_HH, the whole call after the argument checks of sgm_run_impl.  Geometry: ONE stripe over rows [0, h) (no warm-up rows,
// no tiny-image quirk).  Workspace: the 3WAY's buffers only -- the cost volume, and ws.hsum (the 3WAY's L_left + L_right
// volume, same shape) holds S; nothing grows beyond what a 3WAY call of the same size reserves.
// MODE_SGBM (0) would be the same launches with five directions (pass 1 and the row-local right-to-left path).
static int sgm_run_hh(r3d_ctx *ctx, r3d_sgm_ws &ws, hipStream_t st, const r3d_sgbm_params *p, SgmGeom g, const uint8_t *d_left,
                      const uint8_t *d_right, int w, int h, int stride, int16_t *d_disp) {
    g.stripe_sz = h;
    g.overlap = 0;   // the cost kernel's stripe-top blocks (stripes 1..3) then start at row h and own no row
    const size_t npix = (size_t)w * h;
    const size_t rowBytes = (size_t)g.W1 * g.DP * 2, volBytes = rowBytes * h;
    int rc;
    if ((rc = r3d_reserve(ctx, ws.rec_l, npix * 8 * g.CN)) || (rc = r3d_reserve(ctx, ws.rec_r, npix * 8 * g.CN)) ||
        (rc = r3d_reserve(ctx, ws.cost, volBytes)) || (rc = r3d_reserve(ctx, ws.cspec, rowBytes * 3 * (g.SH2 > 0 ? g.SH2 : 1))) ||
        (rc = r3d_reserve(ctx, ws.hsum, volBytes)) || (rc = r3d_reserve(ctx, ws.raw, npix * 2)) ||
        (rc = r3d_reserve(ctx, ws.mins, npix * 2)) || (rc = r3d_reserve(ctx, ws.lrd, npix * 2)) || (rc = r3d_reserve(ctx, ws.flags, 256)))
        return rc;
    ctx->last_w = w; ctx->last_h = h; ctx->last_w1 = g.W1; ctx->last_dp = g.DP;
    ctx->last_mode = p->mode; ctx->last_geom = g;
    r3d_prof_begin(ctx, ws);
    r3d_prof_mark(ctx, ws, st, "prefilter");
    launch_prefilter(st, ws, g, d_left, d_right, stride);
    R3D_HIP(ctx, hipGetLastError());
    r3d_prof_mark(ctx, ws, st, "cost");
    if ((rc = launch_cost2(ctx, ws, g, st))) return rc;   // also the envelope's tracked-maximum pass where it applies
    const float inv_a = 1.0f / (float)(100 - g.uniq);
    for (int r = 0; r < 8; r++) {
        r3d_prof_mark(ctx, ws, st, HH_NAMES[r]);
        launch_hh_path(st, g, r, (const int *)ws.cost.p, (int *)ws.hsum.p, inv_a, (int16_t *)ws.raw.p, (int16_t *)ws.mins.p);
        R3D_HIP(ctx, hipGetLastError());
    }
    r3d_prof_mark(ctx, ws, st, "lrcheck");
    k_lrcheck<<<h, 256, (size_t)w * 4, st>>>((const int16_t *)ws.raw.p, (const int16_t *)ws.mins.p, g, (int16_t *)ws.lrd.p);
    R3D_HIP(ctx, hipGetLastError());
    r3d_prof_mark(ctx, ws, st, "median3");
    k_median3<<<dim3((w + 255) / 256, h), 256, 0, st>>>((const int16_t *)ws.lrd.p, d_disp, w, h);
    R3D_HIP(ctx, hipGetLastError());
    if (p->speckleWindowSize > 0) {
        r3d_prof_mark(ctx, ws, st, "speckles");
        if ((rc = r3d_speckle_run(ctx, ws, st, d_disp, w, h, g.invalid, p->speckleWindowSize, 16 * p->speckleRange))) return rc;
    }
    r3d_prof_end(ctx, ws, st);
    return R3D_OK;
}

// debug / stage parity (r3d_sgbm_debug_hh_partial): directions 0 .. n_dirs-1 again over the cost volume the last MODE_HH call left in
// lane 0's workspace, with the launches of sgm_run_hh (same geometry, grid and direction table), every direction storing: ws.hsum
// then holds S after n_dirs directions.  raw, mins and lrd are not written.  The caller has checked the arguments.
int r3d_sgm_hh_partial(r3d_ctx *ctx, int n_dirs) {
    R3D_HIP(ctx, hipSetDevice(ctx->device));
    r3d_sgm_ws &ws = ctx->ws[0];
    const SgmGeom &g = ctx->last_geom;
    const float inv_a = 1.0f / (float)(100 - g.uniq);
    for (int r = 0; r < n_dirs; r++) {
        launch_hh_path(ctx->stream, g, r, (const int *)ws.cost.p, (int *)ws.hsum.p, inv_a, (int16_t *)ws.raw.p, (int16_t *)ws.mins.p, true);
        R3D_HIP(ctx, hipGetLastError());
    }
    return R3D_OK;
}

// debug / stage parity (r3d_sgbm_debug_select): the selection stage alone on volumes the caller hands in.  Host code around the
// product's launchers: the geometry of a compute call of this size (derive_geom, one channel; MODE_HH: one stripe, as sgm_run_hh),
// the workspace of lane 0 reserved as sgm_run_impl does (the record images, which no kernel here reads, left out), the arrays
// expanded to DP slots per column with the caller's padding values in slots D..DP-1, raw / mins / lrd filled with the invalid
// marker, then launch_vscan2 (3WAY; one pass, no tiny-image second run, no assembly) or the last direction of launch_hh_path
// (HH: r = 7, FOLD 2, ws.hsum as the running S), and k_lrcheck.  Synchronises; the caller copies the planes out.
int r3d_sgm_debug_select(r3d_ctx *ctx, const r3d_sgbm_params *p, int w, int h, const int16_t *cost, const int16_t *cspec,
                         const int16_t *hsum, int cost_pad, int hsum_pad) {
    if (ctx->poisoned) return r3d_fail(ctx, R3D_E_HIP, "context poisoned by an earlier timed-out call: destroy it");
    SgmGeom g;
    if (int rc = derive_geom(ctx, p, w, h, 1, g)) return rc;
    if (!cost || !hsum) return r3d_fail(ctx, R3D_E_BADARG, "debug_select: cost or hsum is NULL");
    if (g.W1 <= 0) return r3d_fail(ctx, R3D_E_BADARG, "debug_select: empty matching range (w1 = %d), no volumes exist", g.W1);
    if (cost_pad < 0 || cost_pad > 16383 || hsum_pad < -32768 || hsum_pad > 32767)
        return r3d_fail(ctx, R3D_E_BADARG, "debug_select: cost_pad %d outside 0..16383 or hsum_pad %d outside int16", cost_pad, hsum_pad);
    const bool hh = p->mode == R3D_SGBM_MODE_HH;
    if (hh) { g.stripe_sz = h; g.overlap = 0; }
    const bool use_cspec = !hh && g.SH2 > 0;
    const size_t D = g.D, DP = g.DP, cols = (size_t)h * g.W1, crows = use_cspec ? (size_t)3 * g.SH2 : 0;
    for (size_t i = 0; i < cols * D; i++)
        if (cost[i] < 0 || cost[i] > 16383)
            return r3d_fail(ctx, R3D_E_BADARG, "debug_select: cost[%zu] = %d outside 0..16383 (the kernels' envelope)", i, (int)cost[i]);
    if (use_cspec && cspec)
        for (size_t i = 0; i < crows * g.W1 * D; i++)
            if (cspec[i] < 0 || cspec[i] > 16383)
                return r3d_fail(ctx, R3D_E_BADARG, "debug_select: cspec[%zu] = %d outside 0..16383 (the kernels' envelope)", i, (int)cspec[i]);
    R3D_HIP(ctx, hipSetDevice(ctx->device));
    r3d_sgm_ws &ws = ctx->ws[0];
    hipStream_t st = ctx->stream;
    const size_t npix = (size_t)w * h, rowBytes = (size_t)g.W1 * DP * 2, volBytes = rowBytes * h;
    int rc;
    if ((rc = r3d_reserve(ctx, ws.cost, volBytes)) || (rc = r3d_reserve(ctx, ws.cspec, rowBytes * 3 * (g.SH2 > 0 ? g.SH2 : 1))) ||
        (rc = r3d_reserve(ctx, ws.raw, npix * 2)) || (rc = r3d_reserve(ctx, ws.mins, npix * 2)) || (rc = r3d_reserve(ctx, ws.lrd, npix * 2)) ||
        (rc = r3d_reserve(ctx, ws.flags, 256)) || (rc = r3d_reserve(ctx, ws.hsum, volBytes)))
        return rc;
    ctx->last_w = w; ctx->last_h = h; ctx->last_w1 = g.W1; ctx->last_dp = g.DP;
    ctx->last_mode = p->mode; ctx->last_geom = g;
    // [columns][D] -> [columns][DP], slots D..DP-1 = pad
    auto expand = [&](const int16_t *src, size_t ncols, int pad) {
        std::vector<int16_t> v(ncols * DP, (int16_t)pad);
        for (size_t c = 0; c < ncols; c++) memcpy(&v[c * DP], src + c * D, D * 2);
        return v;
    };
    const std::vector<int16_t> c_h = expand(cost, cols, cost_pad), h_h = expand(hsum, cols, hsum_pad);
    std::vector<int16_t> s_h;
    if (use_cspec) {
        if (cspec) s_h = expand(cspec, crows * g.W1, cost_pad);
        else {   // what the cost kernel leaves when the box is not replicated: the volume's own rows from the stripe's first row on
            s_h.resize(crows * g.W1 * DP);
            for (int n = 1; n <= 3; n++) {
                const int s0 = std::max(std::min(n * g.stripe_sz - g.overlap, h), 0);
                for (int j = 0; j < g.SH2; j++)
                    memcpy(&s_h[((size_t)(n - 1) * g.SH2 + j) * g.W1 * DP], &c_h[(size_t)std::min(s0 + j, h - 1) * g.W1 * DP], rowBytes);
            }
        }
    }
    R3D_HIP(ctx, hipMemcpyAsync(ws.cost.p, c_h.data(), volBytes, hipMemcpyHostToDevice, st));
    R3D_HIP(ctx, hipMemcpyAsync(ws.hsum.p, h_h.data(), volBytes, hipMemcpyHostToDevice, st));
    if (use_cspec) R3D_HIP(ctx, hipMemcpyAsync(ws.cspec.p, s_h.data(), s_h.size() * 2, hipMemcpyHostToDevice, st));
    const unsigned nb = (unsigned)std::min<size_t>((npix + 255) / 256, 4096);
    for (int16_t *plane : {(int16_t *)ws.raw.p, (int16_t *)ws.mins.p, (int16_t *)ws.lrd.p}) k_fill_s16<<<nb, 256, 0, st>>>(plane, npix, (int16_t)g.invalid);
    R3D_HIP(ctx, hipGetLastError());
    const float inv_a = 1.0f / (float)(100 - g.uniq);
    if (hh) launch_hh_path(st, g, 7, (const int *)ws.cost.p, (int *)ws.hsum.p, inv_a, (int16_t *)ws.raw.p, (int16_t *)ws.mins.p);
    else launch_vscan2(st, g, inv_a, (const int *)ws.cost.p, (const int *)ws.cspec.p, (const int *)ws.hsum.p, (int16_t *)ws.raw.p, (int16_t *)ws.mins.p);
    R3D_HIP(ctx, hipGetLastError());
    k_lrcheck<<<h, 256, (size_t)w * 4, st>>>((const int16_t *)ws.raw.p, (const int16_t *)ws.mins.p, g, (int16_t *)ws.lrd.p);
    R3D_HIP(ctx, hipGetLastError());
    R3D_HIP(ctx, hipStreamSynchronize(st));   // also: the host vectors above outlive their copies
    return R3D_OK;
}

int r3d_streambench_run(r3d_ctx *ctx, int mode, int rows, size_t row_bytes, int write, int delay, int reps, float *ms) {
    R3D_HIP(ctx, hipSetDevice(ctx->device));
    const size_t row_words = row_bytes / 4, bytes = (size_t)rows * row_bytes;
    int rc;
    if ((rc = r3d_reserve(ctx, ctx->ws[0].cost, bytes)) || (rc = r3d_reserve(ctx, ctx->ws[0].hsum, bytes))) return rc;
    r3d_event a, b;
    R3D_HIP(ctx, a.create());
    R3D_HIP(ctx, b.create());
    for (int i = 0; i < reps + 1; i++) {
        if (i == 1) R3D_HIP(ctx, hipEventRecord(a, ctx->stream));
        const int *in = (const int *)ctx->ws[0].cost.p;
        int *out = (int *)ctx->ws[0].hsum.p;
        // mode bit 0: request shape, bit 1: non-temporal loads, bit 2: non-temporal stores
        switch (mode & 7) {
            case 0: k_streambench<0, 0, 0><<<rows, 64, 0, ctx->stream>>>(in, out, row_words, write, delay); break;
            case 1: k_streambench<1, 0, 0><<<rows, 64, 0, ctx->stream>>>(in, out, row_words, write, delay); break;
            case 2: k_streambench<0, 1, 0><<<rows, 64, 0, ctx->stream>>>(in, out, row_words, write, delay); break;
            case 3: k_streambench<1, 1, 0><<<rows, 64, 0, ctx->stream>>>(in, out, row_words, write, delay); break;
            case 4: k_streambench<0, 0, 1><<<rows, 64, 0, ctx->stream>>>(in, out, row_words, write, delay); break;
            case 5: k_streambench<1, 0, 1><<<rows, 64, 0, ctx->stream>>>(in, out, row_words, write, delay); break;
            case 6: k_streambench<0, 1, 1><<<rows, 64, 0, ctx->stream>>>(in, out, row_words, write, delay); break;
            default: k_streambench<1, 1, 1><<<rows, 64, 0, ctx->stream>>>(in, out, row_words, write, delay); break;
        }
    }
    R3D_HIP(ctx, hipEventRecord(b, ctx->stream));
    R3D_HIP(ctx, hipEventSynchronize(b));
    R3D_HIP(ctx, hipEventElapsedTime(ms, a, b));
    *ms /= reps;
    return R3D_OK;
}

int r3d_speckle_run(r3d_ctx *ctx, r3d_sgm_ws &ws, hipStream_t st, int16_t *d_img, int w, int h, int newVal, int maxSize, int maxDiff) {
    const size_t n = (size_t)w * h;
    if (n > 0x7fffffff) return r3d_fail(ctx, R3D_E_UNSUPPORTED, "filterSpeckles: image too large");
    int rc;
    if ((rc = r3d_reserve(ctx, ws.spk_l, n * 4)) || (rc = r3d_reserve(ctx, ws.spk_c, n * 4))) return rc;
    int *L = (int *)ws.spk_l.p, *C = (int *)ws.spk_c.p;
    const int nb = (int)((n + 255) / 256);
    k_spk_init<<<nb, 256, 0, st>>>(d_img, (int)n, newVal, L, C);
    k_spk_merge<<<dim3((w + 255) / 256, h), 256, 0, st>>>(d_img, w, h, newVal, maxDiff, L);
    k_spk_count<<<nb, 256, 0, st>>>((int)n, L, C);
    k_spk_apply<<<nb, 256, 0, st>>>(d_img, (int)n, newVal, maxSize, L, C);
    R3D_HIP(ctx, hipGetLastError());
    return R3D_OK;
}

int r3d_selftest_run(r3d_ctx *ctx) {
    R3D_HIP(ctx, hipSetDevice(ctx->device));
    if (int rc = r3d_reserve(ctx, ctx->ws[0].flags, 256)) return rc;
    R3D_HIP(ctx, hipMemsetAsync(ctx->ws[0].flags.p, 0, 4, ctx->stream));
    k_selftest<<<1, 64, 0, ctx->stream>>>((int *)ctx->ws[0].flags.p);
    R3D_HIP(ctx, hipGetLastError());
    int bad = -1;
    R3D_HIP(ctx, hipMemcpyAsync(&bad, ctx->ws[0].flags.p, 4, hipMemcpyDeviceToHost, ctx->stream));
    R3D_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (bad != 0) return r3d_fail(ctx, R3D_E_HIP, "selftest: cross-lane primitive mismatch, mask=0x%x", bad);
    return R3D_OK;
}

// pass 0: the whole call.  pass 1 (only from pass 0, tiny images): ONE run over the whole image from row 0 (a single stripe), up to
// and including the LR check, its map left in ws.lrd2 -- the rows QUIRK_SMALL_IMAGE_STRIPES hands out in place of a clamped
// stripe's own.
static int sgm_run_impl(r3d_ctx *ctx, int lane, hipStream_t st, const r3d_sgbm_params *p, const uint8_t *d_left, const uint8_t *d_right,
                        int w, int h, int stride, int cn, int16_t *d_disp, int pass);
int r3d_sgm_run(r3d_ctx *ctx, int lane, hipStream_t st, const r3d_sgbm_params *p, const uint8_t *d_left, const uint8_t *d_right,
                int w, int h, int stride, int cn, int16_t *d_disp) {
    return sgm_run_impl(ctx, lane, st, p, d_left, d_right, w, h, stride, cn, d_disp, 0);
}
static int sgm_run_impl(r3d_ctx *ctx, int lane, hipStream_t st, const r3d_sgbm_params *p, const uint8_t *d_left, const uint8_t *d_right,
                        int w, int h, int stride, int cn, int16_t *d_disp, int pass) {
    r3d_sgm_ws &ws = ctx->ws[lane];
    if (ctx->poisoned) return r3d_fail(ctx, R3D_E_HIP, "context poisoned by an earlier timed-out call: destroy it");
    SgmGeom g;
    if (int rc = derive_geom(ctx, p, w, h, cn, g)) return rc;
    if (!d_left || !d_right || !d_disp) return r3d_fail(ctx, R3D_E_BADARG, "sgbm: null image pointer");
    if (stride < w * cn) return r3d_fail(ctx, R3D_E_BADARG, "sgbm: stride %d < width %d x %d channel(s)", stride, w, cn);
    R3D_HIP(ctx, hipSetDevice(ctx->device));
    if (g.W1 <= 0) {  // minX1 >= maxX1: like the original, an all-invalid map, no error
        const size_t np = (size_t)w * h;
        k_fill_s16<<<(unsigned)std::min<size_t>((np + 255) / 256, 4096), 256, 0, st>>>(d_disp, np, (int16_t)((g.minD - 1) * 16));
        R3D_HIP(ctx, hipGetLastError());
        ctx->last_w = w; ctx->last_h = h; ctx->last_w1 = 0; ctx->last_dp = 0;
        ctx->last_mode = p->mode; ctx->last_geom = g;
        return R3D_OK;
    }
    if (p->mode == R3D_SGBM_MODE_HH) return sgm_run_hh(ctx, ws, st, p, g, d_left, d_right, w, h, stride, d_disp);
    const size_t npix = (size_t)w * h;
    const size_t rowBytes = (size_t)g.W1 * g.DP * 2;
    const size_t volBytes = rowBytes * h;
    int rc;
    if ((rc = r3d_reserve(ctx, ws.rec_l, npix * 8 * g.CN))) return rc;   // one record plane per channel
    if ((rc = r3d_reserve(ctx, ws.rec_r, npix * 8 * g.CN))) return rc;
    if ((rc = r3d_reserve(ctx, ws.cost, volBytes))) return rc;
    if ((rc = r3d_reserve(ctx, ws.cspec, rowBytes * 3 * (g.SH2 > 0 ? g.SH2 : 1)))) return rc;
    if ((rc = r3d_reserve(ctx, ws.raw, npix * 2))) return rc;
    if ((rc = r3d_reserve(ctx, ws.mins, npix * 2))) return rc;
    if ((rc = r3d_reserve(ctx, ws.lrd, npix * 2))) return rc;
    // R3D_QUIRK_SMALL_IMAGE_STRIPES=0 places every row of a tiny image at its own position (the rounds 1-3 behaviour)
    static const bool tiny_quirk = [] { const char *e = getenv("R3D_QUIRK_SMALL_IMAGE_STRIPES"); return !(e && !strcmp(e, "0")); }();
    const bool tiny = pass == 0 && tiny_quirk && g.stripe_sz < h && g.stripe_sz - g.overlap < 0;   // stripe 1 exists and its start is clamped
    if (pass == 1) g.stripe_sz = h;                    // one stripe: rows [0, h) from row 0 (the other three own no row)
    if ((tiny || pass == 1) && (rc = r3d_reserve(ctx, ws.lrd2, npix * 2))) return rc;
    ctx->last_w = w; ctx->last_h = h; ctx->last_w1 = g.W1; ctx->last_dp = g.DP;
    ctx->last_mode = p->mode; ctx->last_geom = g;
    if ((rc = r3d_reserve(ctx, ws.flags, 256))) return rc;
    if ((rc = r3d_reserve(ctx, ws.hsum, volBytes))) return rc;   // after the small buffers: the order of first reservation places the two volumes
    r3d_prof_begin(ctx, ws);

    r3d_prof_mark(ctx, ws, st, "prefilter");
    launch_prefilter(st, ws, g, d_left, d_right, stride);
    R3D_HIP(ctx, hipGetLastError());
    r3d_prof_mark(ctx, ws, st, "cost");
    if ((rc = launch_cost2(ctx, ws, g, st))) return rc;
    r3d_prof_mark(ctx, ws, st, "hscan");
    if ((rc = launch_hscan2(ctx, ws, st, g))) return rc;
    r3d_prof_mark(ctx, ws, st, "vscan_wta");
    launch_vscan2(st, g, 1.0f / (float)(100 - g.uniq), (const int *)ws.cost.p, (const int *)ws.cspec.p, (const int *)ws.hsum.p,
                  (int16_t *)ws.raw.p, (int16_t *)ws.mins.p);
    R3D_HIP(ctx, hipGetLastError());
    r3d_prof_mark(ctx, ws, st, "lrcheck");
    k_lrcheck<<<h, 256, (size_t)w * 4, st>>>((const int16_t *)ws.raw.p, (const int16_t *)ws.mins.p, g, (int16_t *)(pass == 1 ? ws.lrd2.p : ws.lrd.p));
    R3D_HIP(ctx, hipGetLastError());
    if (pass == 1) return R3D_OK;
    if (tiny) {
        // second run (workspaces are reused: this pass's LR-checked map is complete in ws.lrd, stream-ordered), then the assembly
        const bool prof = ctx->profiling;
        ctx->profiling = false;
        rc = sgm_run_impl(ctx, lane, st, p, d_left, d_right, w, h, stride, cn, d_disp, 1);
        ctx->profiling = prof;
        if (rc) return rc;
        k_tiny_assemble<<<dim3((w + 255) / 256, h), 256, 0, st>>>((int16_t *)ws.lrd.p, (const int16_t *)ws.lrd2.p, g);
        R3D_HIP(ctx, hipGetLastError());
    }
    r3d_prof_mark(ctx, ws, st, "median3");
    k_median3<<<dim3((w + 255) / 256, h), 256, 0, st>>>((const int16_t *)ws.lrd.p, d_disp, w, h);
    R3D_HIP(ctx, hipGetLastError());
    if (p->speckleWindowSize > 0) {
        r3d_prof_mark(ctx, ws, st, "speckles");
        if ((rc = r3d_speckle_run(ctx, ws, st, d_disp, w, h, g.invalid, p->speckleWindowSize, 16 * p->speckleRange))) return rc;
    }
    r3d_prof_end(ctx, ws, st);
    return R3D_OK;
}
