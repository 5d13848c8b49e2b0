"""The selection stage of the SGM chain -- vertical path, S = sat16(hsum + L_vert), winner-take-all, uniqueness, sub-pixel, the
disp2 scatter and the two-sided LR test -- restated in int64 numpy with Python loops over pixels.  It is lines 97-124 of
tests/sgbm_numpy_ref.py made reusable (and pinned to oracle/sgbm3way.c by tests/test_sgbm_select_ref.py), with the inputs of the
stage as arguments, so that a test can hand the GPU kernels and this file the same crafted volumes.  Every function returns
three int64 [H][W] planes: raw_wta (disparity x16 before the LR check), mins (min_d S at every matched pixel) and lrd (after
the LR check); pixels outside the matching columns hold the invalid marker (minD - 1) * 16 in all three."""
import numpy as np

from tests.sgbm_numpy_ref import step

SHRT_MIN, SHRT_MAX = -32768, 32767


def matching_range(W, minD, D):
    """(minX1, maxX1): the image columns that have a disparity vector."""
    return max(minD + D, 0), W + min(minD, 0)


def width_of(W1, minD, D):
    """The image width whose matching range has W1 columns."""
    return W1 + max(minD + D, 0) - min(minD, 0)


def stripes(H, bs):
    """[(s0, s1, o0)] of the four stripes: rows [s0, s1) are scanned, rows [o0, s1) are the stripe's own."""
    stripe = -(-H // 4)
    overlap = (bs // 2 + 1) + -(-stripe // 10)
    return [(max(min(n * stripe - overlap, H), 0), min((n + 1) * stripe, H), min(n * stripe, H)) for n in range(4)]


def ceil_threshold(minS, uniq):
    """Smallest integer T with T * (100 - uniq) >= minS * 100:  S * (100 - uniq) < minS * 100  <=>  S < T."""
    return -((-int(minS) * 100) // (100 - uniq))


def subpixel(sm, s0, sp):
    """The x16 offset OpenCV adds to an interior winner: C's truncating division."""
    den = max(int(sm + sp - 2 * s0), 1)
    num = int(sm - sp) * 16 + den
    q = abs(num) // (2 * den)
    return q if num >= 0 else -q


def select_from_S(S, W, minD, D, uniq, d12):
    """S: int [H][W1][D], the finished aggregation volume (already saturated to int16)."""
    S = np.asarray(S).astype(np.int64)
    H, W1 = S.shape[:2]
    minX1, maxX1 = matching_range(W, minD, D)
    assert S.shape == (H, W1, D) and W1 == maxX1 - minX1 and SHRT_MIN <= S.min() and S.max() <= SHRT_MAX
    INV = (minD - 1) * 16
    raw = np.full((H, W), INV, np.int64)
    mins = np.full((H, W), INV, np.int64)
    lrd = np.full((H, W), INV, np.int64)
    ds = np.arange(D)
    for y in range(H):
        d2 = np.full(W, INV, np.int64)
        d2c = np.full(W, SHRT_MAX, np.int64)
        for x in range(W1 - 1, -1, -1):                       # right to left, as the original's row loop
            Sx = S[y, x]
            best = int(np.argmin(Sx))                         # the first minimum
            mS = int(Sx[best])
            mins[y, x + minX1] = mS
            if ((Sx * (100 - uniq) < mS * 100) & (np.abs(ds - best) > 1)).any():
                continue
            x2 = x + minX1 - best - minD
            if d2c[x2] > mS:                                  # strict: among equal costs the first visited (largest x) stays
                d2c[x2] = mS
                d2[x2] = best + minD
            dsp = best * 16
            if 0 < best < D - 1:
                dsp += subpixel(Sx[best - 1], mS, Sx[best + 1])
            raw[y, x + minX1] = dsp + minD * 16
        for x in range(minX1, maxX1):
            d1 = int(raw[y, x])
            lrd[y, x] = d1
            if d1 == INV:
                continue
            _d = d1 >> 4
            d_ = (d1 + 15) >> 4
            _x = x - _d
            x_ = x - d_
            # an unset disp2 slot holds INV, which passes ">= minD" when minD >= 2 and then counts as a disagreeing match
            if (0 <= _x < W and d2[_x] >= minD and abs(d2[_x] - _d) > d12 and
                    0 <= x_ < W and d2[x_] >= minD and abs(d2[x_] - d_) > d12):
                lrd[y, x] = INV
    return raw, mins, lrd


def aggregate(costs_of_stripe, Hs, bs, P1, P2):
    """S = clip(Hs + L_vert) [H][W1][D]: per stripe n the vertical chain runs over costs_of_stripe(n, s0, s1) (int [s1-s0][W1][D],
    the cost rows that stripe sees) from zeros at s0; rows from o0 on are the stripe's own."""
    Hs = np.asarray(Hs).astype(np.int64)
    H, W1, D = Hs.shape
    S = np.zeros((H, W1, D), np.int64)
    owned = np.zeros(H, bool)
    for n, (s0, s1, o0) in enumerate(stripes(H, bs)):
        if s0 >= s1:
            continue
        C = np.asarray(costs_of_stripe(n, s0, s1)).astype(np.int64)
        assert C.shape == (s1 - s0, W1, D)
        top = np.zeros((W1, D), np.int64)
        topmin = np.zeros(W1, np.int64)
        for y in range(s0, s1):
            for x in range(W1):
                top[x], topmin[x] = step(C[y - s0, x], top[x], topmin[x], P1, P2)
            if y >= o0:
                assert not owned[y]
                owned[y] = True
                S[y] = np.clip(Hs[y] + top, SHRT_MIN, SHRT_MAX)
    assert owned.all()
    return S


def select(costs_of_stripe, Hs, W, H, minD, D, bs, P1, P2, uniq, d12):
    """MODE_SGBM_3WAY's stage: (raw_wta, mins, lrd).  P1, P2, uniq, d12 are the effective values (after the defaults)."""
    assert np.asarray(Hs).shape[0] == H
    return select_from_S(aggregate(costs_of_stripe, Hs, bs, P1, P2), W, minD, D, uniq, d12)


def select_hh_uniform(S_in, c, W, minD, D, P2, uniq, d12):
    """MODE_HH's last direction fused with the selection, for a cost volume that is uniform in d (c: int [H][W1]).  A path over
    such a volume is L(p) = c(p) - P2 at every disparity: the start has Lp = 0, minp = 0, so min(Lp, Lp + P1, minp + P2) = 0
    and L = c - P2; from then on Lp is uniform, equal to minp, so the min is minp and L = c + minp - (minp + P2).
    Hence S = sat16(S_in + c - P2), in one stripe."""
    S = np.clip(np.asarray(S_in).astype(np.int64) + (np.asarray(c).astype(np.int64) - P2)[:, :, None], SHRT_MIN, SHRT_MAX)
    return select_from_S(S, W, minD, D, uniq, d12)
