"""numpy restatement of the Fast Global Registration contract ("FGR"; [recalled, Open3D 0.18
FastGlobalRegistration.cpp] for the algorithm; the tuple sampler, a pure function of (inputs, options, seed), is this library's).

Steps, for source points S [ns, 3], target points Q [nt, 3] and pairs corres [ncorr, 2] (source index, target index):
 1. normalise: mean_s, mean_t by plain sums in index order / n; both clouds centred; scale = the largest point norm of both;
    use_absolute_scale off: scale_global = scale, scale_start = 1; on: scale_global = 1, scale_start = scale; both / scale_global
 2. pairs: given, or the mutual ones of two nearest-feature searches (mutual_pairs), in ascending source index
 3. tuple test (tuple_test on): trial t < 100 ncorr draws r_j = ransac_ref.sample_index(seed, t, j, ncorr), j < 3; accepted iff
    every edge (r0, r1), (r1, r2), (r2, r0) has li * tuple_scale < lj and lj < li / tuple_scale (li between the source points, lj
    between the target points); the first maximum_tuple_count accepted trials, in t order, give their three pairs each
 4. optimise (M >= 10 rows): par = scale_start, trans = I; per iteration the 6 x 6 Gauss-Newton system of the line-process
    weights s = (par / (|p - trans q0|^2 + par))^2, summed in row order, solved by LDL^T with no determinant rule (a zero pivot
    or a non-finite solution: identity delta), trans = delta trans; par /= division_factor every fourth iteration while
    par > maximum_correspondence_distance
 5. result: T_ts = [R | -R mean_t + t scale_global + mean_s] maps target to source; the result is its rigid inverse.

Recalled quirks, each a switch here (the device implements the True side only):
 QUIRK_UNSCALED_DISTANCE  maximum_correspondence_distance is compared with par as given, although par lives in normalised units
 QUIRK_FEW_PAIRS          with M < 10 the loop is skipped but the result is still de-normalised: the centroid-to-centroid
                          translation, not the identity

`run(..., literal=True)` is the per-pair form for tiny inputs, the default the vectorised one.  A trial is SENSITIVE if one of its
six comparisons lies within BAND = 1e-12 relative of its threshold (edges of a repeated index, 0 < 0, are not: both sides are
exact zeros everywhere)."""
import functools
import math

import numpy as np

from tests import ransac_ref as rr

QUIRK_UNSCALED_DISTANCE = True
QUIRK_FEW_PAIRS = True
BAND = 1e-12
MIN_PAIRS = 10
TRIALS_PER_PAIR = 100
EDGES = ((0, 1), (1, 2), (2, 0))

DEFAULTS = dict(division_factor=1.4, use_absolute_scale=False, decrease_mu=True, maximum_correspondence_distance=0.025,
                iteration_number=64, tuple_scale=0.95, maximum_tuple_count=1000, tuple_test=True, seed=0)


def options(**kw):
    bad = set(kw) - set(DEFAULTS)
    if bad:
        raise TypeError(f"unknown FGR options {sorted(bad)}")
    return dict(DEFAULTS, **kw)


# ---------------------------------------------------------------------------------------------------------------- 1. normalise
def normalise(src, tgt, use_absolute_scale=False, literal=False):
    """(S, Q normalised, dict(mean_s, mean_t, scale, scale_global, scale_start)); scale == 0 raises ValueError"""
    src, tgt = np.asarray(src, np.float64), np.asarray(tgt, np.float64)
    means, cent = [], []
    for c in (src, tgt):
        if literal:
            acc = [0.0, 0.0, 0.0]
            for row in c:
                for a in range(3):
                    acc[a] += float(row[a])
            m = np.array(acc) / len(c)
        else:
            m = np.add.reduce(c, 0) / len(c)                          # an axis-0 reduction adds the rows in index order
        means.append(m)
        cent.append(c - m)
    scale = 0.0
    for c in cent:
        scale = max(scale, float(np.sqrt((c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2]).max()))
    if not scale > 0.0 or not math.isfinite(scale):
        raise ValueError("fgr: scale == 0")
    sg, s0 = (1.0, scale) if use_absolute_scale else (scale, 1.0)
    return cent[0] / sg, cent[1] / sg, dict(mean_s=means[0], mean_t=means[1], scale=scale, scale_global=sg, scale_start=s0)


# -------------------------------------------------------------------------------------------------------------------- 2. pairs
def mutual_pairs(nn_st, nn_ts):
    """the plain cross-check of two nearest-neighbour tables: (i, nn_st[i]) with nn_ts[nn_st[i]] == i, ascending i"""
    nn_st, nn_ts = np.asarray(nn_st), np.asarray(nn_ts)
    i = np.arange(len(nn_st))
    keep = nn_ts[nn_st] == i
    return np.stack([i[keep], nn_st[keep]], 1).astype(np.int32)


# ---------------------------------------------------------------------------------------------------------------- 3. tuple test
def _edge_len(d):
    return np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])


def tuple_trials(p, q, t0, count, tuple_scale, seed):
    """trials t0 .. t0 + count - 1 over the normalised pair points p, q [ncorr, 3]:
    (samples int32 [count, 3], flags int32 [count], sensitive bool [count])"""
    ncorr = len(p)
    c = rr.samples(seed, t0, count, 3, ncorr)[:, :3]
    ok = np.ones(count, bool)
    sens = np.zeros(count, bool)
    for a, b in EDGES:
        li = _edge_len(p[c[:, a]] - p[c[:, b]])
        lj = _edge_len(q[c[:, a]] - q[c[:, b]])
        lo, hi = li * tuple_scale, li / tuple_scale
        ok &= (lo < lj) & (lj < hi)
        live = ~((li == 0) & (lj == 0))
        sens |= live & ((np.abs(lo - lj) <= BAND * np.maximum(lj, lo)) | (np.abs(hi - lj) <= BAND * np.maximum(lj, hi)))
    return c, ok.astype(np.int32), sens


def tuple_trial_literal(p, q, t, tuple_scale, seed):
    """one trial, step by step: (sample list, flag)"""
    ncorr = len(p)
    c = [rr.sample_index(seed, t, j, ncorr) for j in range(3)]
    for a, b in EDGES:
        d, e = p[c[a]] - p[c[b]], q[c[a]] - q[c[b]]
        li = math.sqrt((float(d[0]) * float(d[0]) + float(d[1]) * float(d[1])) + float(d[2]) * float(d[2]))
        lj = math.sqrt((float(e[0]) * float(e[0]) + float(e[1]) * float(e[1])) + float(e[2]) * float(e[2]))
        if not (li * tuple_scale < lj and lj < li / tuple_scale):
            return c, 0
    return c, 1


def tuple_test(p, q, tuple_scale, maximum_tuple_count, seed, literal=False, chunk=65536):
    """dict(index int64 [3 tuples]: the accepted trials' pair indices in t order up to the cut; tuples; trials = the trial that
    fills the last place + 1, or 100 ncorr when the count is never reached; sensitive: the in-band trials among those)"""
    ncorr = len(p)
    total = TRIALS_PER_PAIR * ncorr
    picked, sens, trials = [], 0, total
    t0 = 0
    while t0 < total and len(picked) < maximum_tuple_count:
        cnt = min(chunk, total - t0)
        if literal:
            rows = [tuple_trial_literal(p, q, t0 + i, tuple_scale, seed) for i in range(cnt)]
            c, ok, sn = np.array([r[0] for r in rows], np.int32), np.array([r[1] for r in rows], np.int32), np.zeros(cnt, bool)
        else:
            c, ok, sn = tuple_trials(p, q, t0, cnt, tuple_scale, seed)
        acc = np.nonzero(ok)[0]
        room = maximum_tuple_count - len(picked)
        if len(acc) >= room:                                         # the cut falls inside this chunk
            acc = acc[:room]
            trials = t0 + int(acc[-1]) + 1
            sens += int(sn[:acc[-1] + 1].sum())
        else:
            sens += int(sn.sum())
        picked.extend(c[acc].tolist())
        t0 += cnt
    idx = np.array(picked, np.int64).reshape(-1, 3)
    return dict(index=idx.reshape(-1), tuples=len(idx), trials=trials, sensitive=sens)


# ------------------------------------------------------------------------------------------------------------------ 4. optimise
def ldlt_solve(a, b):
    """x = A \\ b by the LDL^T of the library's solve6_to_matrix, operation by operation, without its determinant rule:
    None for a zero pivot or a non-finite x"""
    n = 6
    lo = [[0.0] * n for _ in range(n)]
    dg = [0.0] * n
    for j in range(n):
        d = float(a[j][j])
        for k in range(j):
            d -= lo[j][k] * lo[j][k] * dg[k]
        dg[j] = d
        lo[j][j] = 1.0
        for i in range(j + 1, n):
            v = float(a[i][j])
            for k in range(j):
                v -= lo[i][k] * lo[j][k] * dg[k]
            lo[i][j] = v / d if d != 0 else 0.0
    if any(d == 0 for d in dg):
        return None
    y = [0.0] * n
    for i in range(n):
        y[i] = float(b[i])
        for k in range(i):
            y[i] -= lo[i][k] * y[k]
    for i in range(n):
        y[i] /= dg[i]
    x = [0.0] * n
    for i in range(n - 1, -1, -1):
        x[i] = y[i]
        for k in range(i + 1, n):
            x[i] -= lo[k][i] * x[k]
    return x if all(math.isfinite(v) for v in x) else None


def delta_matrix(x):
    """TransformVector6dToMatrix4d: Rz(x2) Ry(x1) Rx(x0), translation x3..5"""
    sa, ca, sb, cb, sc, cc = math.sin(x[0]), math.cos(x[0]), math.sin(x[1]), math.cos(x[1]), math.sin(x[2]), math.cos(x[2])
    d = np.eye(4)
    d[:3, :3] = [[cc * cb, cc * sb * sa - sc * ca, cc * sb * ca + sc * sa], [sc * cb, sc * sb * sa + cc * ca, sc * sb * ca - cc * sa],
                 [-sb, cb * sa, cb * ca]]
    d[:3, 3] = x[3:6]
    return d


def mat4_mul(a, b):
    """the library's mat4_mul: every entry summed over k in ascending order from 0"""
    out = np.zeros((4, 4))
    for i in range(4):
        for j in range(4):
            s = 0.0
            for k in range(4):
                s += float(a[i, k]) * float(b[k, j])
            out[i, j] = s
    return out


# the 27 sums as 16 distinct ones (the others are their exact negatives, the sum of s itself, or sums of exact zeros):
# [A00 A01 A02 A11 A12 A22 | S s qx, S s qy, S s qz | S s | b0 .. b5]
def _terms(p, q, par):
    rx, ry, rz = p[..., 0] - q[..., 0], p[..., 1] - q[..., 1], p[..., 2] - q[..., 2]
    qx, qy, qz = q[..., 0], q[..., 1], q[..., 2]
    w = par / (((rx * rx + ry * ry) + rz * rz) + par)
    s = w * w
    return [s * (qy * qy + qz * qz), s * -(qx * qy), s * -(qx * qz), s * (qx * qx + qz * qz), s * -(qy * qz), s * (qx * qx + qy * qy),
            s * qx, s * qy, s * qz, s,
            s * (qz * ry - qy * rz), s * (qx * rz - qz * rx), s * (qy * rx - qx * ry), s * -rx, s * -ry, s * -rz]


def system_from_sums(v):
    """(JTJ [6, 6], JTr [6]) of the 16 sums"""
    a00, a01, a02, a11, a12, a22, sx, sy, sz, ss = v[:10]
    a = np.array([[a00, a01, a02, 0.0, -sz, sy], [a01, a11, a12, sz, 0.0, -sx], [a02, a12, a22, -sy, sx, 0.0],
                  [0.0, sz, -sy, ss, 0.0, 0.0], [-sz, 0.0, sx, 0.0, ss, 0.0], [sy, -sx, 0.0, 0.0, 0.0, ss]])
    return a, np.array(v[10:16])


def apply_trans(trans, q0):
    """trans q0: every coordinate ((r0 x + r1 y) + r2 z) + t"""
    x, y, z = q0[..., 0], q0[..., 1], q0[..., 2]
    return np.stack([((trans[i, 0] * x + trans[i, 1] * y) + trans[i, 2] * z) + trans[i, 3] for i in range(3)], -1)


def optimise(rows, scale_start, maximum_correspondence_distance, division_factor=1.4, iteration_number=64, decrease_mu=True,
             scale_global=1.0, literal=False, reverse=False):
    """step 4 on normalised pair rows [M, 6] (p, q0): (trans [4, 4], par, trace_T [iterations, 4, 4], trace_par [iterations],
    failed: the iterations whose solve gave the identity delta).  reverse: the sums taken in descending row order."""
    rows = np.asarray(rows, np.float64).reshape(-1, 6)
    trans, par = np.eye(4), float(scale_start)
    trace_t, trace_p, failed = np.zeros((iteration_number, 4, 4)), np.zeros(iteration_number), []
    if len(rows) < MIN_PAIRS:
        return trans, par, trace_t[:0], trace_p[:0], failed
    limit = maximum_correspondence_distance if QUIRK_UNSCALED_DISTANCE else maximum_correspondence_distance / scale_global
    p, q0 = rows[:, :3], rows[:, 3:]
    order = range(len(rows) - 1, -1, -1) if reverse else range(len(rows))
    for itr in range(iteration_number):
        if literal:
            v = [0.0] * 16
            for i in order:
                t = _terms(p[i], apply_trans(trans, q0[i]), par)
                for e in range(16):
                    v[e] += float(t[e])
        else:
            t = np.stack(_terms(p, apply_trans(trans, q0), par), 1)    # [M, 16]
            v = np.add.reduce(t[::-1] if reverse else t, 0).tolist()   # rows added one by one in that order
        a, b = system_from_sums(v)
        x = ldlt_solve(a, -b)
        if x is None:
            failed.append(itr)
        else:
            trans = mat4_mul(delta_matrix(x), trans)
        if decrease_mu and itr % 4 == 0 and par > limit:
            par /= division_factor
        trace_t[itr], trace_p[itr] = trans, par
    return trans, par, trace_t, trace_p, failed


# -------------------------------------------------------------------------------------------------------------------- 5. result
def original_scale(trans, nrm):
    """the source -> target transform in the clouds' own units"""
    r, t = trans[:3, :3], trans[:3, 3]
    mt, ms, sg = nrm["mean_t"], nrm["mean_s"], nrm["scale_global"]
    tt = np.array([(t[i] * sg - ((r[i, 0] * mt[0] + r[i, 1] * mt[1]) + r[i, 2] * mt[2])) + ms[i] for i in range(3)])
    out = np.eye(4)
    out[:3, :3] = r.T
    out[:3, 3] = [-((r[0, i] * tt[0] + r[1, i] * tt[1]) + r[2, i] * tt[2]) for i in range(3)]
    return out


def run(src, tgt, corres, literal=False, **kw):
    """steps 1, 3, 4, 5 on given pairs: dict(T, matched, trials, tuples, pairs, final_par, rows [M, 6], index (into corres, or
    None), scale_global, scale_start, trace_T, trace_par, sensitive, failed)"""
    o = options(**kw)
    corres = np.asarray(corres).reshape(-1, 2)
    s, q, nrm = normalise(src, tgt, o["use_absolute_scale"], literal)
    p, qq = s[corres[:, 0]], q[corres[:, 1]]
    if o["tuple_test"]:
        tt = tuple_test(p, qq, o["tuple_scale"], o["maximum_tuple_count"], o["seed"], literal) if len(corres) else \
            dict(index=np.zeros(0, np.int64), tuples=0, trials=0, sensitive=0)
        index = tt["index"]
        rows = np.concatenate([p[index], qq[index]], 1)
    else:
        tt, index = dict(tuples=0, trials=0, sensitive=0), None
        rows = np.concatenate([p, qq], 1)
    trans, par, tr_t, tr_p, failed = optimise(rows, nrm["scale_start"], o["maximum_correspondence_distance"], o["division_factor"],
                                              o["iteration_number"], o["decrease_mu"], nrm["scale_global"], literal)
    if len(rows) < MIN_PAIRS and not QUIRK_FEW_PAIRS:
        t4 = np.eye(4)
    else:
        t4 = original_scale(trans, nrm)
    return dict(T=t4, matched=len(corres), trials=tt["trials"], tuples=tt["tuples"], pairs=len(rows), final_par=par, rows=rows,
                index=index, scale_global=nrm["scale_global"], scale_start=nrm["scale_start"], trace_T=tr_t, trace_par=tr_p,
                sensitive=tt["sensitive"], failed=failed, trans=trans)


# ---- the cases tests/test_fgr_gpu.py compares (tests/test_fgr_ref.py checks the conditions on each)
TRIAL_SEED = 7
PLANTED = {"planted600": (600, 220), "planted257": (257, 30), "planted2000": (2000, 416)}
# (accepted trials of all 100 ncorr, the trial that fills the 1000th place or None) recorded with the contract
PLANTED_EXPECT = {"planted600": (3095, 18431), "planted257": (39, None), "planted2000": (2114, 96060)}
TUPLE_CASES = {
    # name: (ncorr, t0, count, tuple_scale)
    "n1": (1, 0, 64, 0.95), "n3": (3, 0, 4096, 0.95), "n63": (63, 0, 4096, 0.95), "n64": (64, 0, 4096, 0.95),
    "n65": (65, 1234567, 4096, 0.95), "n600": (600, 0, 4096, 0.95), "t0_count1": (600, 1234567, 1, 0.95),
    "t0_count63": (600, 1234567, 63, 0.95), "count64": (600, 0, 64, 0.95), "t0_count65": (600, 1234567, 65, 0.95),
    "scale1": (600, 0, 4096, 1.0),
}
TRACE_M = (9, 10, 1023, 1024, 1025, 3000)
# (M, options of the loop plus trace_case's grid / big)
TRACE_CASES = [(m, {}) for m in TRACE_M] + [
    (1025, dict(iteration_number=0)), (1025, dict(iteration_number=1)), (1024, dict(decrease_mu=False)),
    (1023, dict(use_absolute_scale=True, grid=True, big="source")), (3000, dict(use_absolute_scale=True, grid=True, big="target")),
    (10, dict(big="target", division_factor=2.0, maximum_correspondence_distance=0.1)),
]
TRACE_IDS = [f"M{m}-" + "-".join(f"{k}={v}" for k, v in kw.items()) for m, kw in TRACE_CASES]


@functools.lru_cache(maxsize=None)
def planted(name):
    m, ni = PLANTED[name]
    src, tgt, corres, t_true, is_planted = rr.planted_case(m, ni, seed=1000 + m + 3)
    for a in (src, tgt, corres, t_true, is_planted):
        a.setflags(write=False)
    return src, tgt, corres, t_true, is_planted


def pairs_case(ncorr):
    """the first ncorr pairs of a planted case large enough to hold them"""
    m = max(ncorr, 16)
    src, tgt, corres, _, _ = rr.planted_case(m, max(m // 3, 1), seed=1000 + m + 3)
    return src, tgt, corres[:ncorr]


def trace_case(m, grid=False, big="source", extra=37):
    """M pairs over clouds of different sizes (ns = M + extra, nt = M); the point of the largest norm lies in `big`.
    grid: coordinates rounded to multiples of 2^-20, so that every order of summation gives the same means (and the same scale:
    the use_absolute_scale trace is compared bit for bit in par)."""
    src, tgt, corres, _, _ = rr.planted_case(m + extra, (m + extra) // 2, seed=5000 + m)
    keep = np.nonzero(corres[:, 1] < m)[0][:m]
    corres, tgt = corres[keep], tgt[:m].copy()                        # every target index occurs once: exactly m pairs stay
    src = src.copy()
    far = np.array([3.0, -2.5, 2.0])
    if big == "source":
        src[0] += far
    else:
        tgt[0] += far
    if grid:
        src, tgt = np.round(src * 2.0 ** 20) / 2.0 ** 20, np.round(tgt * 2.0 ** 20) / 2.0 ** 20
    return src, tgt, np.ascontiguousarray(corres)
