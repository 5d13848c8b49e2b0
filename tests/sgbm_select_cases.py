"""The catalogue of crafted S vectors for the selection-stage tests (tests/test_sgbm_select_gpu.py part A), and the coverage it
reaches as counted from the reference alone (tests/test_sgbm_select_ref.py asserts it, so that the GPU comparison is known to
pass through the sub-pixel, uniqueness-threshold, rail and LR code).  No GPU here.

One case = one numDisparities with its uniquenessRatio / minDisparity / disp12MaxDiff / P2.  The vectors are laid row-major
into W1 = 37 columns (no multiple of any columns-per-wave count) as the volume S_in; the cost plane is uniform in d, so both
modes see S = sat16(S_in + c - P2) (tests/sgbm_select_ref.py, select_hh_uniform).  Three runs per case:
  zero    c = 0:          the catalogue shifted down by P2 (a path over zero cost is -P2)
  exact   c = P2:         S = S_in, every crafted threshold, tie and rail exactly as built
  random  c in [0, 16383] per pixel: shifts both ways, saturation at both rails (the upper one needs c > P2)
"""
import functools

import numpy as np

from tests import sgbm_select_ref as ref

W1 = 37
BS = 5
#        D   uniq minD  d12  P1    P2
CASES = [(16, 15, 0, 1, 600, 2400),
         (32, 0, -7, 3, 1, 2),
         (48, 5, 5, -1, 4000, 16383),
         (64, 40, -63, 1, 600, 2400),
         (80, 99, 0, 3, 4000, 16383),
         (96, 1, -7, -1, 1, 2),
         (112, 15, 5, 1, 600, 2400),
         (128, 99, -127, 3, 4000, 16383),
         (144, 5, 0, -1, 1, 2),
         (256, 40, -7, 1, 600, 2400),
         (272, 1, 5, 3, 1, 2),
         (512, 15, -511, -1, 4000, 16383)]
RUNS = ("zero", "exact", "random")
SMALL = [(1, 16), (16, 16), (1, 128), (16, 128), (1, 512), (16, 512)]      # (W1, D): one column, one full wave of the 16-column mappings


def case_of(D):
    return next(c for c in CASES if c[0] == D)


def _sat(v):
    return int(min(max(v, ref.SHRT_MIN), ref.SHRT_MAX))


# (sm - minS, sp - minS) that give each sub-pixel offset -7 .. 8; any common positive factor leaves the offset unchanged.  sm > minS
# (an equal entry before the winner would be the first minimum); sp = minS occurs (offset 8: a tie after the winner).
_OFFSET_PAIRS = {}
for _a in range(1, 41):
    for _b in range(0, 41):
        _OFFSET_PAIRS.setdefault(ref.subpixel(_a, 0, _b), (_a, _b))
assert sorted(_OFFSET_PAIRS) == list(range(-7, 9))


def catalogue(D, uniq, seed):
    """int64 [n][D], every entry inside int16."""
    rng = np.random.default_rng(seed)
    out = []

    def far(minS):
        """A rest that neither wins nor counts against uniqueness (unless T itself passes int16): the top 2000 values of int16,
        so that it stays such a rest when a run shifts the whole vector (a shifted minimum moves T by more than the shift)."""
        lo = max(ref.ceil_threshold(minS, uniq), minS) + 200
        return np.minimum(max(lo, ref.SHRT_MAX - 2000) + rng.integers(0, 2000, D), ref.SHRT_MAX)

    # winner sweep: a unique winner at every d, neighbours that walk through all sixteen sub-pixel offsets; one cost per sweep,
    # so that consecutive columns land on ONE disp2 slot with equal cost
    for s, minS in enumerate((100, -2000) if D <= 128 else (100,)):
        for d in range(D):
            v = far(minS)
            a, b = _OFFSET_PAIRS[(d + 5 * s) % 16 - 7]
            m = int(rng.integers(1, 12))
            v[d] = minS
            if d > 0:
                v[d - 1] = minS + a * m
            if d < D - 1:
                v[d + 1] = minS + b * m
            out.append(v)
    # rivals around the uniqueness threshold
    winners = sorted({w for w in (0, 1, 7, 8, 15, 16, 17, D // 2 - 1, D // 2, D - 17, D - 16, D - 2, D - 1) if 0 <= w < D})
    for w in winners:
        for r in sorted({r for r in (w - 16, w - 8, w - 2, w - 1, w + 1, w + 2, w + 8, w + 16, 0, D - 1) if 0 <= r < D and r != w}):
            for minS in (-9000, -1, 0, 1, 37, 9000):
                T = ref.ceil_threshold(minS, uniq)
                for rv in (T - 1, T, T + 1):
                    v = far(minS)
                    v[w] = minS
                    v[r] = _sat(rv)
                    out.append(v)
    # the winner's own neighbours around the threshold together with one rival: the kernels count every S < T and take the
    # neighbourhood's share off again, so the two counts must treat a value at T alike
    for w in sorted({w for w in (1, 8, 15, 16, D // 2, D - 2) if 0 < w < D - 1}):
        r = w + 8 if w + 8 < D else w - 8
        for minS in (1, 37, 9000):
            T = ref.ceil_threshold(minS, uniq)
            for sm in (T - 1, T, T + 1):
                for sp in (T - 1, T, T + 1):
                    for rv in (T - 1, T):
                        v = far(minS)
                        v[w], v[w - 1], v[w + 1], v[r] = minS, _sat(sm), _sat(sp), _sat(rv)
                        out.append(v)
    # extreme minima against a flat rest
    for i, minS in enumerate((-32768, -32767, -32766, -328, -327, 327, 328, 329, 27851, 27852, 32766, 32767)):
        for rest in (minS, minS + 1, ref.ceil_threshold(minS, uniq), 32767):
            v = np.full(D, _sat(rest), np.int64)
            v[(7 * i + 3) % D] = minS
            out.append(v)
    # ties: the first minimum wins
    for i, j in ((3, D - 2), (7, 8), (0, D - 1), (D - 2, D - 1), (D // 2 - 1, D // 2)):
        v = far(50)
        v[i] = v[j] = 50
        out.append(v)
    for b in (1, D // 2, D - 3):
        v = far(-70)
        v[b:] = -70
        out.append(v)
    for d in (1, 8, D - 2):             # the flattest neighbourhood a first minimum can have: denominator 1
        v = far(-5)
        v[d - 1], v[d], v[d + 1] = -4, -5, -5
        out.append(v)
    for i in (0, 5, 7, D - 2):
        v = np.full(D, 32767, np.int64)
        v[i] = v[i + 1] = -32768
        out.append(v)
    out += [np.zeros(D, np.int64), np.full(D, 32767, np.int64), np.full(D, -32768, np.int64)]
    # random
    out += list(rng.integers(-32768, 32768, (64, D)))
    out += list(rng.integers(-300, 301, (64, D)))
    cat = np.array(out, np.int64)
    assert cat.min() >= ref.SHRT_MIN and cat.max() <= ref.SHRT_MAX
    return cat


def _ro(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def volume(D, w1=W1):
    """(S_in int16 [h][w1][D], c_random int16 [h][w1]) of the case with this D; unused pixels hold 32767."""
    _, uniq, *_ = case_of(D)
    cat = catalogue(D, uniq, seed=D)
    if w1 != W1:                        # the small-width runs take an evenly spaced sample of the catalogue
        cat = cat[::max(len(cat) // (8 * w1), 1)][:8 * w1]
    h = -(-len(cat) // w1)
    S_in = np.full((h * w1, D), 32767, np.int16)
    S_in[:len(cat)] = cat
    c = np.random.default_rng(1000 + D + w1).integers(0, 16384, (h, w1)).astype(np.int16)
    return _ro(S_in.reshape(h, w1, D)), _ro(c)


def run_cost(D, run, w1=W1):
    """int16 [h][w1]: the per-pixel cost of a run."""
    S_in, c = volume(D, w1)
    if run == "random":
        return c
    return _ro(np.full(c.shape, 0 if run == "zero" else case_of(D)[5], np.int16))


@functools.lru_cache(maxsize=None)
def expected(D, run, w1=W1):
    """(raw_wta, mins, lrd) int64 [h][W] of one run, from the reference."""
    _, uniq, minD, d12, P1, P2 = case_of(D)
    S_in, _ = volume(D, w1)
    return tuple(_ro(p) for p in ref.select_hh_uniform(S_in, run_cost(D, run, w1), ref.width_of(w1, minD, D), minD, D, P2,
                                                       uniq, d12 if d12 > 0 else 1))


def coverage(D, run):
    """Counts of the regimes a run reaches, from the reference alone."""
    _, uniq, minD, d12, P1, P2 = case_of(D)
    S_in, _ = volume(D)
    c = run_cost(D, run).astype(np.int64)
    pre = S_in.astype(np.int64) + (c - P2)[:, :, None]
    S = np.clip(pre, ref.SHRT_MIN, ref.SHRT_MAX)
    raw, mins, lrd = expected(D, run)
    W = raw.shape[1]
    x0, x1 = ref.matching_range(W, minD, D)
    INV = (minD - 1) * 16
    raw, mins, lrd = raw[:, x0:x1], mins[:, x0:x1], lrd[:, x0:x1]
    assert np.array_equal(mins, S.min(axis=2))
    T = np.array([[ref.ceil_threshold(m, uniq) for m in row] for row in mins])
    valid = raw != INV
    best = S.argmin(axis=2)
    interior = valid & (best > 0) & (best < D - 1)
    offs = (raw - minD * 16 - best * 16)[interior]
    d = np.arange(D)
    flat = np.take_along_axis(S, np.clip(best - 1, 0, D - 1)[..., None], 2)[..., 0] + \
        np.take_along_axis(S, np.clip(best + 1, 0, D - 1)[..., None], 2)[..., 0] - 2 * mins <= 1
    lane = {}
    for width in (8, 16, 32):           # disparities per lane of the mappings in use: winners on both sides of a lane boundary
        lane[width] = (int((valid & (best % width == 0) & (best > 0)).sum()), int((valid & (best % width == width - 1) & (best < D - 1)).sum()))
    return dict(pixels=int(valid.size), invalid_after_wta=float((~valid).mean()), lr_rejected=int((valid & (lrd == INV)).sum()),
                T_above_int16=int((T > 32767).sum()), T_below_int16=int((T < -32768).sum()),
                rival_at_T=int(((S == T[..., None]) & (np.abs(d - best[..., None]) > 1)).any(axis=2).sum()),
                rival_below_T=int(((S == T[..., None] - 1) & (np.abs(d - best[..., None]) > 1)).any(axis=2).sum()),
                sat_low=int((pre < ref.SHRT_MIN).any(axis=2).sum()), sat_high=int((pre > ref.SHRT_MAX).any(axis=2).sum()),
                minS_negative=int((mins < 0).sum()), winners=int(np.unique(best[valid]).size),
                winner_first=int((valid & (best == 0)).sum()), winner_last=int((valid & (best == D - 1)).sum()),
                offsets=sorted(set(int(o) for o in offs)), ties=int(((S == mins[..., None]).sum(axis=2) > 1).sum()),
                flat_denominator=int((interior & flat).sum()), lane_edges=lane,
                slot_collisions=_collisions(raw, mins, best, minD, INV))


def _collisions(raw, mins, best, minD, INV):
    """Pairs of valid pixels of one row that land on the same disp2 slot with equal cost."""
    n = 0
    for y in range(raw.shape[0]):
        seen = {}
        for x in range(raw.shape[1]):
            if raw[y, x] != INV:
                k = (x - int(best[y, x]), int(mins[y, x]))
                n += seen.get(k, 0)
                seen[k] = seen.get(k, 0) + 1
    return n
