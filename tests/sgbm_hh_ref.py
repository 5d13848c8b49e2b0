"""Restatement of SGBM MODE_HH (OpenCV 4.x computeDisparitySGBM with fullDP = true) in numpy.

Written from the contract of the MODE_HH issue ([recalled], like SURVEY.md Appendix A), not from the kernels:
  * C is the 3WAY block cost of ONE stripe covering rows [0, H): oracle.sgbm_oracle.cost_rows(L, R, params, 0, 0, H);
  * every direction r (predecessor q = p - r) runs  L_r(p) = C(p) + min(Lq, Lq[d-1]+P1, Lq[d+1]+P1, mq+P2) - (mq+P2),
    Lq[-1] = Lq[D] = SHRT_MAX, and a predecessor outside [0,W1)x[0,H) has L = 0, m = 0;
  * S folds the eight directions in the order of DIRECTIONS with one saturating int16 add per direction (the CV_SIMD
    build); QUIRK_HH_SUM_ORDER = "scalar" selects the scalar fallback (one saturating add of the four terms, summed in
    int, per pass);
  * WTA (first minimum), uniqueness, sub-pixel, the disp2 scatter (x descending, strict '>'), the two-sided LR check,
    medianBlur(3) and filterSpeckles (oracle.sgbm_oracle.filter_speckles) as in 3WAY.

compute() is vectorised over lines x disparities (C2 on the host in a few minutes); compute_literal() is shaped like
OpenCV's pass / row / x loop with the two Lr row buffers and is meant for tiny images only.  They share nothing after C.
"""
import numpy as np

SHRT_MAX, SHRT_MIN = 32767, -32768
DISP_SHIFT, DISP_SCALE = 4, 16
NR2 = 4   # directions per pass

# QUIRK_HH_SUM_ORDER: "simd" (default; what the product reproduces) or "scalar"
QUIRK_HH_SUM_ORDER = "simd"
SUM_ORDERS = ("simd", "scalar")

# path directions r = p - q, in the order they enter S
PASS1 = ((1, 0), (1, 1), (0, 1), (-1, 1))      # rows top->bottom, x ascending: q = (x-1,y), (x-1,y-1), (x,y-1), (x+1,y-1)
PASS2 = ((-1, 0), (1, -1), (0, -1), (-1, -1))  # rows bottom->top, x descending: q = (x+1,y), (x-1,y+1), (x,y+1), (x+1,y+1)
DIRECTIONS = PASS1 + PASS2


def derive(W, minDisparity=0, numDisparities=16, blockSize=3, P1=0, P2=0, disp12MaxDiff=0, preFilterCap=0,
           uniquenessRatio=0, speckleWindowSize=0, speckleRange=0):
    """The derived parameters of 3WAY (SURVEY.md Appendix A 'derive')."""
    minD, D = minDisparity, numDisparities
    assert D > 0 and D % 16 == 0
    P1 = P1 if P1 > 0 else 2
    P2 = max(P2 if P2 > 0 else 5, P1 + 1)
    maxD = minD + D
    minX1, maxX1 = max(maxD, 0), W + min(minD, 0)
    return dict(minD=minD, D=D, P1=P1, P2=P2, minX1=minX1, maxX1=maxX1, W1=maxX1 - minX1,
                uniq=uniquenessRatio if uniquenessRatio >= 0 else 10, d12=disp12MaxDiff if disp12MaxDiff > 0 else 1,
                INV=(minD - 1) * DISP_SCALE, speckleWindowSize=speckleWindowSize, speckleRange=speckleRange)


def block_cost(L, R, kw):
    """C[y][xc][d] (int16): the 3WAY block cost of one stripe over rows [0, H) (oracle/sgbm3way.c's QUIRKs included)."""
    from oracle import sgbm_oracle as so
    H = L.shape[0]
    return so.cost_rows(L, R, so.make_params(**kw), 0, 0, H)


def _sat16(a):
    return np.clip(a, SHRT_MIN, SHRT_MAX)


def _step(C, Lp, mp, P1, P2):
    """One path step for n independent lines: C, Lp int32 [n, D], mp int32 [n] -> (L, min_d L)."""
    nb = np.empty_like(Lp)
    nb[:, 1:-1] = np.minimum(Lp[:, :-2], Lp[:, 2:])
    nb[:, 0] = np.minimum(SHRT_MAX, Lp[:, 1])
    nb[:, -1] = np.minimum(Lp[:, -2], SHRT_MAX)
    nb += P1
    mp2 = (mp + P2)[:, None]
    Lr = C + np.minimum(np.minimum(Lp, mp2), nb) - mp2
    return Lr, Lr.min(axis=1)


def _direction(C, r, P1, P2, fold):
    """Runs direction r over the whole volume and hands every line-slice of L_r to fold(index, L)."""
    H, W1, D = C.shape
    dx, dy = r
    if dy == 0:   # rows: all H lines at once, loop over x
        Lp, mp = np.zeros((H, D), np.int32), np.zeros(H, np.int32)
        for x in (range(W1) if dx > 0 else range(W1 - 1, -1, -1)):
            Lp, mp = _step(C[:, x].astype(np.int32), Lp, mp, P1, P2)
            fold((slice(None), x), Lp)
        return
    # columns and both diagonals: loop over y; row y's predecessors are row y-dy shifted by dx
    prevL, prevm = np.zeros((W1, D), np.int32), np.zeros(W1, np.int32)
    for y in (range(H) if dy > 0 else range(H - 1, -1, -1)):
        if dx == 0:
            Lp, mp = prevL, prevm
        else:
            Lp, mp = np.zeros((W1, D), np.int32), np.zeros(W1, np.int32)
            if dx > 0:
                Lp[1:], mp[1:] = prevL[:-1], prevm[:-1]
            else:
                Lp[:-1], mp[:-1] = prevL[1:], prevm[1:]
        prevL, prevm = _step(C[y].astype(np.int32), Lp, mp, P1, P2)
        fold((y,), prevL)


def aggregate(C, P1, P2, sum_order=None):
    """S (int16 [H, W1, D]) of the eight directions folded in contract order."""
    sum_order = sum_order or QUIRK_HH_SUM_ORDER
    assert sum_order in SUM_ORDERS
    S = np.zeros(C.shape, np.int16)
    for dirs in (PASS1, PASS2):
        if sum_order == "simd":
            def fold(i, Lr):
                S[i] = _sat16(S[i].astype(np.int32) + Lr)
            for r in dirs:
                _direction(C, r, P1, P2, fold)
        else:
            T = np.zeros(C.shape, np.int32)

            def fold(i, Lr):
                T[i] += Lr
            for r in dirs:
                _direction(C, r, P1, P2, fold)
            S[:] = _sat16(S.astype(np.int32) + T)
    return S


def direction_volume(C, r, P1, P2):
    """L_r (int32 [H, W1, D]) of the one direction r: _direction with a fold that stores."""
    Lr = np.zeros(C.shape, np.int32)

    def fold(i, L):
        Lr[i] = L
    _direction(C, r, P1, P2, fold)
    return Lr


def partial_sums(C, P1, P2):
    """[S_1 .. S_8] (int16 [H, W1, D] each): S after the first n directions, "simd" order (one saturating add per direction)."""
    out, S = [], np.zeros(C.shape, np.int32)
    for r in DIRECTIONS:
        S = _sat16(S + direction_volume(C, r, P1, P2))
        out.append(S.astype(np.int16))
    return out


def _trunc_div(n, d):
    q = np.abs(n) // d
    return np.where(n >= 0, q, -q)


def select(S, g, W, rows=64):
    """WTA + uniqueness + sub-pixel + disp2 scatter + LR check -> the raw (LR-checked, pre-median) map int16 [H, W]."""
    H, W1, D = S.shape
    minD, minX1, maxX1, INV = g["minD"], g["minX1"], g["maxX1"], g["INV"]
    out = np.full((H, W), INV, np.int16)
    dd = np.arange(D)
    X = np.arange(minX1, maxX1)
    for y0 in range(0, H, rows):
        Si = S[y0:y0 + rows].astype(np.int32)
        h = Si.shape[0]
        best = Si.argmin(axis=2)
        minS = np.take_along_axis(Si, best[..., None], 2)[..., 0]
        bad = np.zeros(best.shape, bool)
        if g["uniq"] > 0:
            bad = ((Si * (100 - g["uniq"]) < minS[..., None] * 100) & (np.abs(dd - best[..., None]) > 1)).any(axis=2)
        sm = np.take_along_axis(Si, np.maximum(best - 1, 0)[..., None], 2)[..., 0]
        sp = np.take_along_axis(Si, np.minimum(best + 1, D - 1)[..., None], 2)[..., 0]
        den = np.maximum(sm + sp - 2 * minS, 1)
        inner = (best > 0) & (best < D - 1)
        dsp = best * DISP_SCALE + np.where(inner, _trunc_div((sm - sp) * DISP_SCALE + den, 2 * den), 0) + minD * DISP_SCALE
        d1 = np.where(bad, INV, dsp)
        # disp2: lowest cost wins; among equal costs the first in x-descending order (the largest x)
        x2 = X[None, :] - best - minD
        key = np.full((h, W), np.iinfo(np.int64).max, np.int64)
        ok = ~bad
        yy = np.broadcast_to(np.arange(h)[:, None], best.shape)
        xc = np.broadcast_to(np.arange(W1)[None, :], best.shape)
        np.minimum.at(key, (yy[ok], x2[ok]), minS[ok].astype(np.int64) * W1 + (W1 - 1 - xc[ok]))
        seen = key != np.iinfo(np.int64).max
        d2 = np.where(seen, (W1 - 1 - key % W1) + minX1 - np.arange(W)[None, :], INV)
        # two-sided LR check
        _d = d1 >> DISP_SHIFT
        d_ = (d1 + DISP_SCALE - 1) >> DISP_SHIFT

        def disagrees(xx, dv):
            inside = (xx >= 0) & (xx < W)
            v = np.take_along_axis(d2, np.clip(xx, 0, W - 1), 1)
            return inside & (v >= minD) & (np.abs(v - dv) > g["d12"])
        lr_bad = (d1 != INV) & disagrees(X[None, :] - _d, _d) & disagrees(X[None, :] - d_, d_)
        out[y0:y0 + h, minX1:maxX1] = np.where(lr_bad, INV, d1)
    return out


def median3(a):
    H, W = a.shape
    p = np.pad(a, 1, mode="edge")
    return np.sort(np.stack([p[i:i + H, j:j + W] for i in range(3) for j in range(3)]), axis=0)[4]


def finish(raw, g):
    from oracle import sgbm_oracle as so
    med = median3(raw)
    if g["speckleWindowSize"] > 0:
        med = so.filter_speckles(med, g["INV"], g["speckleWindowSize"], 16 * g["speckleRange"])
    return med


def compute(L, R, sum_order=None, return_raw=False, return_S=False, **kw):
    """Vectorised restatement.  kw: cv2.StereoSGBM_create's keyword names (mode omitted).  Returns the final int16 map
    (and the raw map / S on request)."""
    H, W = L.shape
    g = derive(W, **kw)
    if g["W1"] <= 0:
        full = np.full((H, W), g["INV"], np.int16)
        return (full, full.copy()) if return_raw else full
    S = aggregate(block_cost(L, R, kw), g["P1"], g["P2"], sum_order)
    raw = select(S, g, W)
    out = [finish(raw, g)]
    if return_raw:
        out.append(raw)
    if return_S:
        out.append(S)
    return out[0] if len(out) == 1 else tuple(out)


def compute_literal(L, R, sum_order=None, return_raw=False, **kw):
    """Literal restatement: OpenCV's loop structure, per pixel, with two Lr row buffers per pass.  Tiny images only."""
    sum_order = sum_order or QUIRK_HH_SUM_ORDER
    H, W = L.shape
    g = derive(W, **kw)
    INV, minD, D, P1, P2, minX1, W1 = g["INV"], g["minD"], g["D"], g["P1"], g["P2"], g["minX1"], g["W1"]
    disp1 = np.full((H, W), INV, np.int64)
    if W1 <= 0:
        return (disp1.astype(np.int16),) * 2 if return_raw else disp1.astype(np.int16)
    C = block_cost(L, R, kw).astype(np.int64)
    S = np.zeros((H, W1, D), np.int64)

    def path(Lp, mp, c):
        Lq = np.concatenate([[SHRT_MAX], Lp, [SHRT_MAX]])
        out = np.empty(D, np.int64)
        for d in range(D):
            out[d] = c[d] + min(Lq[d + 1], Lq[d] + P1, Lq[d + 2] + P1, mp + P2) - (mp + P2)
        return out

    for pas in (1, 2):
        ys = range(H) if pas == 1 else range(H - 1, -1, -1)
        xs = range(W1) if pas == 1 else range(W1 - 1, -1, -1)
        dx = 1 if pas == 1 else -1
        # Lr[x + 1][r]: entries 0 and W1 + 1 stay zero (a predecessor outside the image has L = 0 and min 0)
        Lr_prev, min_prev = np.zeros((W1 + 2, NR2, D), np.int64), np.zeros((W1 + 2, NR2), np.int64)
        for y in ys:
            Lr_cur, min_cur = np.zeros((W1 + 2, NR2, D), np.int64), np.zeros((W1 + 2, NR2), np.int64)
            disp2 = np.full(W, INV, np.int64)
            disp2cost = np.full(W, SHRT_MAX, np.int64)
            for x in xs:
                i = x + 1
                preds = ((Lr_cur[i - dx, 0], min_cur[i - dx, 0]),   # r0: the previous pixel of this row
                         (Lr_prev[i - 1, 1], min_prev[i - 1, 1]),   # r1: q = (x-1, previous row)
                         (Lr_prev[i, 2], min_prev[i, 2]),           # r2: q = (x,   previous row)
                         (Lr_prev[i + 1, 3], min_prev[i + 1, 3]))   # r3: q = (x+1, previous row)
                terms = []
                for r, (Lp, mp) in enumerate(preds):
                    Lr = path(Lp, int(mp), C[y, x])
                    assert SHRT_MIN <= Lr.min() and Lr.max() <= SHRT_MAX
                    Lr_cur[i, r], min_cur[i, r] = Lr, Lr.min()
                    terms.append(Lr)
                if sum_order == "simd":
                    for Lr in terms:
                        S[y, x] = np.clip(S[y, x] + Lr, SHRT_MIN, SHRT_MAX)
                else:
                    S[y, x] = np.clip(S[y, x] + terms[0] + terms[1] + terms[2] + terms[3], SHRT_MIN, SHRT_MAX)
                if pas == 1:
                    continue
                Sp = S[y, x]
                minS, best = SHRT_MAX + 1, -1
                for d in range(D):
                    if Sp[d] < minS:
                        minS, best = int(Sp[d]), d
                if g["uniq"] > 0 and any(Sp[d] * (100 - g["uniq"]) < minS * 100 and abs(best - d) > 1 for d in range(D)):
                    continue
                d = best
                x2 = x + minX1 - d - minD
                if disp2cost[x2] > minS:
                    disp2cost[x2] = minS
                    disp2[x2] = d + minD
                if 0 < d < D - 1:
                    den = max(int(Sp[d - 1] + Sp[d + 1] - 2 * Sp[d]), 1)
                    num = int(Sp[d - 1] - Sp[d + 1]) * DISP_SCALE + den
                    q = abs(num) // (2 * den)
                    d = d * DISP_SCALE + (q if num >= 0 else -q)
                else:
                    d *= DISP_SCALE
                disp1[y, x + minX1] = d + minD * DISP_SCALE
            Lr_prev, min_prev = Lr_cur, min_cur
            if pas == 1:
                continue
            for x in range(minX1, g["maxX1"]):
                d1 = int(disp1[y, x])
                if d1 == INV:
                    continue
                _d = d1 >> DISP_SHIFT
                d_ = (d1 + DISP_SCALE - 1) >> DISP_SHIFT
                _x, x_ = x - _d, x - d_
                if (0 <= _x < W and disp2[_x] >= minD and abs(disp2[_x] - _d) > g["d12"] and
                        0 <= x_ < W and disp2[x_] >= minD and abs(disp2[x_] - d_) > g["d12"]):
                    disp1[y, x] = INV
    raw = disp1.astype(np.int16)
    med = finish(raw, g)
    return (med, raw) if return_raw else med
