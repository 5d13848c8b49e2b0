"""Restatement of the FPFH contract of DESIGN.md section 4 ("FPFH"; Open3D 0.18 Feature.cpp, recalled) in numpy / plain Python,
float64, no GPU.  Written from the contract, not from the kernels.

Rows are [n][33] (the C ABI's layout).  Neighbour lists come from tests/neighbor_ref.brute_knn: self first, nearest first, ties
by index, d2 < radius*radius, padded with -1.

Two forms that share nothing after the neighbour lists:
    fpfh_vectorised  numpy over all points at once, one neighbour slot at a time
    fpfh_literal     a loop per point and per neighbour over Python floats (math.sqrt / acos / atan2), for tiny clouds
Both spell the arithmetic out in the contract's order: x*x + y*y + z*z (never a library norm), sums taken sequentially.

Both also return, per point, the number of SENSITIVE pairs: pairs whose binning or role swap another correct libm (the device's
acos / atan2) may decide differently:
    a pre-floor bin coordinate within 1e-9 of an interior edge 1 .. 10,
    0 < ||a1| - |a2|| < 1e-9     (acos has slope >= 1 in magnitude: a wider gap cannot flip),
    0 < |v| < 1e-9 * f3."""
import math

import numpy as np

from tests import neighbor_ref as nr

DIM = 33
PI = math.pi
EDGE = 1e-9


def neighbors(points, radius, max_nn):
    """(idx [n,k] int32 padded with -1, d2 [n,k]) of the hybrid search (radius None or <= 0: plain kNN), k = min(max_nn, n):
    neighbor_ref.brute_knn(points, points, k, radius)'s lists -- the same distance expression and the same (d2, index) order --
    without sorting whole rows: the k-th smallest distance of a row bounds its candidates (ties included), and only those are
    sorted.  tests/test_fpfh_ref.py compares the two."""
    p = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
    n, k = len(p), min(int(max_nn), len(p))
    idx = np.full((n, k), -1, np.int32)
    d2 = np.full((n, k), nr.PAD_D2)
    r2 = radius * radius if radius is not None and radius > 0 else np.inf
    for b in range(0, n, nr.CHUNK):
        D = nr._pair_d2(p, p[b:b + nr.CHUNK])
        kth = np.partition(D, k - 1, axis=1)[:, k - 1]
        for r in range(len(D)):
            c = np.flatnonzero((D[r] <= kth[r]) & (D[r] < r2))
            c = c[np.lexsort((c, D[r, c]))][:k]
            idx[b + r, :len(c)] = c
            d2[b + r, :len(c)] = D[r, c]
    return idx, d2


# ------------------------------------------------------------------------------------------------------------- literal form
def _pair_literal(p1, n1, p2, n2):
    """(f0, f1, f2, sensitive) of one pair, contract steps 1-7"""
    dx, dy, dz = p2[0] - p1[0], p2[1] - p1[1], p2[2] - p1[2]
    f3 = math.sqrt(dx * dx + dy * dy + dz * dz)
    if f3 == 0.0:
        return 0.0, 0.0, 0.0, False
    a1 = (n1[0] * dx + n1[1] * dy + n1[2] * dz) / f3
    a2 = (n2[0] * dx + n2[1] * dy + n2[2] * dz) / f3
    gap = abs(abs(a1) - abs(a2))
    sens = 0.0 < gap < EDGE

    def acos(x):
        return math.acos(x) if x <= 1.0 else math.nan          # |a| can exceed 1 by a rounding: no swap then

    if acos(abs(a1)) > acos(abs(a2)):
        m1, m2 = n2, n1
        dx, dy, dz = -dx, -dy, -dz
        f2 = -a2
    else:
        m1, m2 = n1, n2
        f2 = a1
    vx, vy, vz = dy * m1[2] - dz * m1[1], dz * m1[0] - dx * m1[2], dx * m1[1] - dy * m1[0]
    vn = math.sqrt(vx * vx + vy * vy + vz * vz)
    if vn == 0.0:
        return 0.0, 0.0, 0.0, sens
    if vn < EDGE * f3:
        sens = True
    vx, vy, vz = vx / vn, vy / vn, vz / vn
    wx, wy, wz = m1[1] * vz - m1[2] * vy, m1[2] * vx - m1[0] * vz, m1[0] * vy - m1[1] * vx
    f1 = vx * m2[0] + vy * m2[1] + vz * m2[2]
    f0 = math.atan2(wx * m2[0] + wy * m2[1] + wz * m2[2], m1[0] * m2[0] + m1[1] * m2[1] + m1[2] * m2[2])
    return f0, f1, f2, sens


def _bin_literal(c):
    """(bin 0 .. 10, near an interior edge)"""
    b = math.floor(c)
    near = abs(c - round(c)) < EDGE and 1 <= round(c) <= 10
    return min(max(b, 0), 10), near


def fpfh_literal(points, normals, radius, max_nn, nbrs=None):
    """(spfh [n,33], fpfh [n,33], sensitive [n]) by the contract, one point and one neighbour at a time"""
    p = [tuple(float(v) for v in r) for r in np.asarray(points, np.float64).reshape(-1, 3)]
    nm = [tuple(float(v) for v in r) for r in np.asarray(normals, np.float64).reshape(-1, 3)]
    idx, d2 = nbrs if nbrs is not None else neighbors(points, radius, max_nn)
    n = len(p)
    spfh = [[0.0] * DIM for _ in range(n)]
    sens = [0] * n
    for i in range(n):
        nb = [int(j) for j in idx[i] if j >= 0]
        nn = len(nb)
        if nn <= 1:
            continue
        h = 100.0 / (nn - 1)
        for j in nb[1:]:
            f0, f1, f2, s = _pair_literal(p[i], nm[i], p[j], nm[j])
            b0, e0 = _bin_literal(11 * (f0 + PI) / (2.0 * PI))
            b1, e1 = _bin_literal(11 * (f1 + 1.0) / 2)
            b2, e2 = _bin_literal(11 * (f2 + 1.0) / 2)
            spfh[i][b0] += h
            spfh[i][11 + b1] += h
            spfh[i][22 + b2] += h
            sens[i] += bool(s or e0 or e1 or e2)
    fpfh = fpfh_stage_literal(spfh, idx, d2)
    return np.array(spfh).reshape(n, DIM), fpfh, np.array(sens, np.int64)


def fpfh_stage_literal(spfh, idx, d2):
    """the second stage on given SPFH rows"""
    n = len(idx)
    out = np.zeros((n, DIM))
    for i in range(n):
        acc = [0.0] * DIM
        tot = [0.0, 0.0, 0.0]
        for k in range(1, idx.shape[1]):
            j = int(idx[i, k])
            if j < 0:
                break
            dist = float(d2[i, k])
            if dist == 0.0:
                continue
            for q in range(DIM):
                val = float(spfh[j][q]) / dist
                tot[q // 11] += val
                acc[q] += val
        for g in range(3):
            if tot[g] != 0.0:
                tot[g] = 100.0 / tot[g]
        for q in range(DIM):
            out[i, q] = acc[q] * tot[q // 11] + float(spfh[i][q])
    return out


# ---------------------------------------------------------------------------------------------------------- vectorised form
def _near_edge(c):
    r = np.rint(c)
    return (np.abs(c - r) < EDGE) & (r >= 1) & (r <= 10)


def _bins(c):
    with np.errstate(invalid="ignore"):
        return np.clip(np.nan_to_num(np.floor(c), nan=0.0), 0, 10).astype(np.int64)


def spfh_vectorised(points, normals, idx):
    """(spfh [n,33], sensitive [n]): all points at once, neighbour slot by neighbour slot (the order of the contract's sum)"""
    p = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
    nm = np.ascontiguousarray(normals, np.float64).reshape(-1, 3)
    n = len(p)
    spfh = np.zeros((n, DIM))
    sens = np.zeros(n, np.int64)
    nn = (idx >= 0).sum(1)
    h = np.where(nn > 1, 100.0 / np.maximum(nn - 1, 1), 0.0)
    rows = np.arange(n)
    for k in range(1, idx.shape[1]):
        use = idx[:, k] >= 0
        if not use.any():
            break
        i, j = rows[use], idx[use, k]
        d = p[j] - p[i]
        dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
        n1x, n1y, n1z = nm[i, 0], nm[i, 1], nm[i, 2]
        n2x, n2y, n2z = nm[j, 0], nm[j, 1], nm[j, 2]
        f3 = np.sqrt(dx * dx + dy * dy + dz * dz)
        zero = f3 == 0.0
        f3s = np.where(zero, 1.0, f3)
        a1 = (n1x * dx + n1y * dy + n1z * dz) / f3s
        a2 = (n2x * dx + n2y * dy + n2z * dz) / f3s
        gap = np.abs(np.abs(a1) - np.abs(a2))
        s = ~zero & (gap > 0) & (gap < EDGE)
        with np.errstate(invalid="ignore"):
            swap = np.arccos(np.abs(a1)) > np.arccos(np.abs(a2))
        m1x, m1y, m1z = np.where(swap, n2x, n1x), np.where(swap, n2y, n1y), np.where(swap, n2z, n1z)
        m2x, m2y, m2z = np.where(swap, n1x, n2x), np.where(swap, n1y, n2y), np.where(swap, n1z, n2z)
        dx, dy, dz = np.where(swap, -dx, dx), np.where(swap, -dy, dy), np.where(swap, -dz, dz)
        f2 = np.where(swap, -a2, a1)
        vx, vy, vz = dy * m1z - dz * m1y, dz * m1x - dx * m1z, dx * m1y - dy * m1x
        vn = np.sqrt(vx * vx + vy * vy + vz * vz)
        zero |= vn == 0.0
        s |= ~zero & (vn < EDGE * f3)
        vns = np.where(zero, 1.0, vn)
        vx, vy, vz = vx / vns, vy / vns, vz / vns
        wx, wy, wz = m1y * vz - m1z * vy, m1z * vx - m1x * vz, m1x * vy - m1y * vx
        f1 = vx * m2x + vy * m2y + vz * m2z
        f0 = np.arctan2(wx * m2x + wy * m2y + wz * m2z, m1x * m2x + m1y * m2y + m1z * m2z)
        f0, f1, f2 = np.where(zero, 0.0, f0), np.where(zero, 0.0, f1), np.where(zero, 0.0, f2)
        c0, c1, c2 = 11 * (f0 + PI) / (2.0 * PI), 11 * (f1 + 1.0) / 2, 11 * (f2 + 1.0) / 2
        s |= _near_edge(c0) | _near_edge(c1) | _near_edge(c2)
        spfh[i, _bins(c0)] += h[i]                    # a row occurs once per slot: plain fancy += is an ordinary add
        spfh[i, 11 + _bins(c1)] += h[i]
        spfh[i, 22 + _bins(c2)] += h[i]
        sens[i] += s
    return spfh, sens


def fpfh_stage_vectorised(spfh, idx, d2):
    """the second stage on given SPFH rows [n,33]"""
    spfh = np.ascontiguousarray(spfh, np.float64)
    n = len(idx)
    acc = np.zeros((n, DIM))
    tot = np.zeros((n, 3))
    for k in range(1, idx.shape[1]):
        use = (idx[:, k] >= 0) & (d2[:, k] != 0.0)
        if not (idx[:, k] >= 0).any():
            break
        val = np.where(use[:, None], spfh[np.where(use, idx[:, k], 0)] / np.where(use, d2[:, k], 1.0)[:, None], 0.0)
        for q in range(DIM):                         # sum[q / 11] += val_q, in q order
            tot[:, q // 11] = tot[:, q // 11] + val[:, q]
        acc = acc + val
    scale = np.where(tot != 0.0, 100.0 / np.where(tot != 0.0, tot, 1.0), tot)
    return acc * np.repeat(scale, 11, axis=1) + spfh


def fpfh_vectorised(points, normals, radius, max_nn, nbrs=None):
    """(spfh [n,33], fpfh [n,33], sensitive [n])"""
    idx, d2 = nbrs if nbrs is not None else neighbors(points, radius, max_nn)
    spfh, sens = spfh_vectorised(points, normals, idx)
    return spfh, fpfh_stage_vectorised(spfh, idx, d2), sens


# ------------------------------------------------------------------------------------------------------------ correspondences
def matches_ref(src, tgt, chunk=128):
    """(nn [ns] int32, d2 [ns]): the target row with the smallest sum_j (a_j - b_j)^2, 33 terms added in j order; the first
    minimum = the smaller index on ties.  src, tgt: [n][33] rows."""
    s = np.ascontiguousarray(src, np.float64)
    t = np.ascontiguousarray(tgt, np.float64)
    tt = np.ascontiguousarray(t.T)
    nn = np.empty(len(s), np.int32)
    d2 = np.empty(len(s))
    for b in range(0, len(s), chunk):
        blk = s[b:b + chunk]
        acc = np.zeros((len(blk), len(t)))
        for j in range(s.shape[1]):
            d = blk[:, j, None] - tt[j][None, :]
            acc = acc + d * d
        a = acc.argmin(1)
        nn[b:b + chunk] = a
        d2[b:b + chunk] = acc[np.arange(len(a)), a]
    return nn, d2


def row_distance(src, tgt, nn):
    """sum_j (src[i][j] - tgt[nn[i]][j])^2 in j order, for given pairs"""
    s = np.ascontiguousarray(src, np.float64)
    t = np.ascontiguousarray(tgt, np.float64)[nn]
    acc = np.zeros(len(s))
    for j in range(s.shape[1]):
        d = s[:, j] - t[:, j]
        acc = acc + d * d
    return acc


def correspondences_ref(src, tgt, mutual_filter=False, mutual_consistent_ratio=0.1):
    """int32 [M,2]: (i, nearest target of i); with the mutual filter only pairs whose target's nearest source is i, unless fewer
    than ratio * ns survive (then the unfiltered list)"""
    nn_st, _ = matches_ref(src, tgt)
    ns = len(nn_st)
    corres = np.stack([np.arange(ns, dtype=np.int32), nn_st], 1)
    if not mutual_filter:
        return corres
    nn_ts, _ = matches_ref(tgt, src)
    kept = np.array([(i, j) for i, j in corres if nn_ts[j] == i], np.int32).reshape(-1, 2)
    return corres if len(kept) < mutual_consistent_ratio * ns else kept
