"""GPU tests of the feature-matching RANSAC (r3d_ransac_correspondence, r3d_ransac_correspondence_dev,
r3d_debug_ransac_hypotheses and the Python functions over them) against the numpy restatement in tests/ransac_ref.py.

Bars (per hypothesis).  Samples are integer arithmetic: exact.  A hypothesis that is neither ILL-CONDITIONED (sample covariance
sigma_2 < 1e-6 sigma_1) nor SENSITIVE (a tested quantity within 1e-8 of its threshold) agrees in its flags and its inlier count
exactly, in T to 1e-9 absolute per entry and in err2 to 1e-9 relative: float64 rounding amplified by at most sigma_1 / sigma_2 <=
1e6 gives 1e-10 on clouds of unit scale, and the 1e-8 band covers that error times coordinates up to about 3.  An
ill-conditioned hypothesis is compared in its sample and its edge flag only (and its T must be finite and orthonormal to 1e-12);
a sensitive one may differ in flags or count by its number of in-band items.  tests/test_ransac_ref.py checks that those loose
hypotheses stay under 2 % of every case here (the M = 3 case: that they are exactly the repeated-index samples).

Measured on the MI355X over the 20 per-hypothesis cases: samples, flags and counts equal everywhere; max |dT| 1.6e-12; max relative
err2 difference 3.1e-10; every transform orthonormal to below 1e-12, the rank 0 and rank 1 samples included."""
import ctypes
import functools

import numpy as np
import pytest

from tests import ransac_ref as rr

pytestmark = pytest.mark.gpu
_vp = ctypes.c_void_p


@functools.lru_cache(maxsize=None)
def _ref(name):
    src, tgt, corres, kw = rr.parity_case(name)
    hy = rr.hypotheses(src, tgt, corres, **kw)
    for a in (src, tgt, corres, *hy.values()):
        a.setflags(write=False)
    return src, tgt, corres, kw, hy


def _dev_kw(kw):
    return dict(h0=kw["h0"], count=kw["count"], max_correspondence_distance=kw["max_dist"], ransac_n=kw["n"], edge_length=kw["edge"],
                checker_distance=kw["checker_distance"], seed=kw["seed"])


def _orthonormal(t):
    r = t[:, :, :3]
    return np.abs(np.einsum("bij,bkj->bik", r, r) - np.eye(3)).reshape(len(t), -1).max(1)


@pytest.mark.parametrize("name", sorted(rr.PARITY_CASES))
def test_hypotheses_match_the_restatement(r3d, name):
    src, tgt, corres, kw, hy = _ref(name)
    got = r3d.cloud_ops.debug_ransac_hypotheses(src, tgt, corres, **_dev_kw(kw))
    assert np.array_equal(got["samples"], hy["samples"])
    edge_sens = hy["sens_flags"] > 0
    assert np.array_equal(got["flags"][~edge_sens] & 1, hy["flags"][~edge_sens] & 1)
    has_t = (got["flags"] & 1) != 0
    assert np.isfinite(got["T"]).all() and np.isfinite(got["err2"]).all()
    assert (got["T"][~has_t] == 0).all()
    assert _orthonormal(got["T"][has_t]).max(initial=0.0) < 1e-12
    assert np.allclose(np.linalg.det(got["T"][has_t][:, :, :3]), 1.0)
    strict = ~hy["ill"] & ~edge_sens
    assert np.array_equal(got["flags"][strict], hy["flags"][strict])
    st_t = strict & has_t
    terr = np.abs(got["T"][st_t] - hy["T"][st_t]).max(initial=0.0)
    live = strict & (hy["flags"] == 3)
    dcount = np.abs(got["inliers"][live].astype(np.int64) - hy["inliers"][live])
    exact = live & (hy["sens_pairs"] == 0)
    rel = np.abs(got["err2"][exact] - hy["err2"][exact]) / np.maximum(hy["err2"][exact], 1e-300)
    rel = np.where(hy["err2"][exact] == 0, np.abs(got["err2"][exact]), rel)
    print(f"{name}: {kw['count']} hypotheses, {has_t.sum()} with a transform, {live.sum()} scored, {(~strict).sum()} loose; "
          f"max |dT| {terr:.2e}, max count difference {dcount.max(initial=0)}, max relative err2 difference {rel.max(initial=0.0):.2e}")
    assert terr < 1e-9
    assert (dcount <= hy["sens_pairs"][live]).all()
    assert rel.max(initial=0.0) < 1e-9
    dead = strict & (hy["flags"] != 3)
    assert (got["inliers"][dead] == 0).all() and (got["err2"][dead] == 0).all()
    if name == "coincident":                                         # rank 0 and rank 1 samples really went through
        in_cluster = (hy["samples"][:, :3] < rr.COINCIDENT_PAIRS).sum(1)
        assert (hy["ill"] & has_t & (in_cluster == 3)).any() and (hy["ill"] & has_t & (in_cluster == 2)).any()


def _full(r3d, src, tgt, corres, n=3, edge=0.9, cd=rr.MAX_DIST, max_iteration=8192, confidence=0.999, seed=0, batch=0):
    return r3d.registration_ransac_based_on_correspondence(src, tgt, corres, rr.MAX_DIST, ransac_n=n, edge_length=edge, checker_distance=cd,
                                                           max_iteration=max_iteration, confidence=confidence, seed=seed, batch=batch)


def _check_against_run(res, ref, src, tgt, corres, max_dist=rr.MAX_DIST):
    assert res["iterations"] == ref["iterations"]
    assert abs(res["validated"] - ref["validated"]) <= ref["sens_hypotheses"]
    assert abs(res["inliers"] - ref["inliers"]) <= ref["sens_pairs"]
    assert abs(res["fitness"] - ref["fitness"]) <= ref["sens_pairs"] / len(corres) + 1e-15
    assert res["best_hypothesis"] in ref["equivalent"]
    t_ref = ref["equivalent"][res["best_hypothesis"]]
    assert np.abs(res["T"][:3] - t_ref).max() < 1e-9 and np.array_equal(res["T"][3], [0, 0, 0, 1])
    assert abs(res["inlier_rmse"] - ref["inlier_rmse"]) <= 1e-9 * ref["inlier_rmse"] or ref["sens_pairs"] > 0
    # the returned pairs are the inliers under the returned T (numpy), outside the band
    p, q = src[corres[:, 0]], tgt[corres[:, 1]]
    d = np.sqrt(((p @ res["T"][:3, :3].T + res["T"][:3, 3] - q) ** 2).sum(1))
    key = lambda c: c[:, 0].astype(np.int64) << 32 | c[:, 1].astype(np.int64)       # noqa: E731
    mask = np.isin(key(corres), key(res["correspondence_set"]))
    band = np.abs(d - max_dist) < rr.BAND
    assert np.array_equal(mask[~band], (d < max_dist)[~band])
    assert len(res["correspondence_set"]) == res["inliers"]


@pytest.mark.parametrize("name", ["planted600", "planted2000", "planted257", "n4", "no_edge", "no_checker"])
def test_full_run_matches_the_restatement(r3d, name):
    m, ni, n, edge, cd, _, count = rr.PARITY_CASES[name]
    src, tgt, corres, t_true, planted = rr.planted_case(m, ni, seed=m + n)
    count = min(count, 2048) if name in ("no_edge", "no_checker") else count
    ref = rr.run(src, tgt, corres, rr.MAX_DIST, n, edge, cd, max_iteration=count, confidence=0.999, seed=0)
    res = _full(r3d, src, tgt, corres, n, edge, cd, count)
    _check_against_run(res, ref, src, tgt, corres)
    assert res["inliers"] == ni and np.array_equal(res["correspondence_set"], corres[planted])    # the planted set, exactly
    assert np.abs(res["T"] - t_true).max() < 0.005
    assert res["iterations"] < count and res["setup_ms"] > 0 and res["loop_ms"] > 0


def test_batch_size_never_changes_the_result(r3d):
    src, tgt, corres, _, _ = rr.planted_case(2000, 416, seed=2003)
    for conf, max_it in ((0.999, 8192), (1.0, 3000)):
        runs = [_full(r3d, src, tgt, corres, max_iteration=max_it, confidence=conf, batch=b) for b in (64, 1000, 0)]
        for r in runs[1:]:
            for k in ("best_hypothesis", "iterations", "validated", "inliers", "fitness", "inlier_rmse"):
                assert r[k] == runs[0][k], k
            assert r["T"].tobytes() == runs[0]["T"].tobytes()
            assert np.array_equal(r["correspondence_set"], runs[0]["correspondence_set"])
        assert runs[0]["iterations"] == (765 if conf < 1 else 3000)
    one = _full(r3d, src, tgt, corres, max_iteration=300, confidence=1.0, batch=1)     # a batch of one hypothesis, and an oversized one
    big = _full(r3d, src, tgt, corres, max_iteration=300, confidence=1.0, batch=2 ** 30)
    assert one["T"].tobytes() == big["T"].tobytes() and one["best_hypothesis"] == big["best_hypothesis"] and one["validated"] == big["validated"]


def test_seed_decides_the_run(r3d):
    src, tgt, corres, _, _ = rr.planted_case(600, 220, seed=603)
    a, b, c = (_full(r3d, src, tgt, corres, max_iteration=4096, seed=s) for s in (0, 0, 1))
    for k in ("best_hypothesis", "iterations", "validated", "inliers", "fitness", "inlier_rmse"):
        assert a[k] == b[k]
    assert a["T"].tobytes() == b["T"].tobytes() and np.array_equal(a["correspondence_set"], b["correspondence_set"])
    # many samples find all 220 planted pairs: which one comes first depends on the seed
    refs = [rr.run(src, tgt, corres, rr.MAX_DIST, 3, 0.9, rr.MAX_DIST, max_iteration=4096, seed=s) for s in (0, 1)]
    assert refs[0]["best_hypothesis"] != refs[1]["best_hypothesis"]
    assert a["best_hypothesis"] != c["best_hypothesis"] and a["inliers"] == c["inliers"] == 220
    _check_against_run(c, refs[1], src, tgt, corres)


def test_empty_outcomes(r3d):
    src, tgt, corres, _, _ = rr.planted_case(600, 220, seed=603)
    ident = np.stack([np.arange(600), np.arange(600)], 1).astype(np.int32)
    res = _full(r3d, src, tgt[::-1].copy(), ident, edge=0.999, max_iteration=300)    # pure outliers: nothing passes the edge checker
    assert res["best_hypothesis"] == -1 and res["fitness"] == 0 and res["inlier_rmse"] == 0 and res["inliers"] == 0
    assert np.array_equal(res["T"], np.eye(4)) and res["iterations"] == 300 and res["validated"] == 0
    assert res["correspondence_set"].shape == (0, 2)
    # batches of 32 with no survivor and with one survivor in the middle of a run
    hy = rr.hypotheses(src, tgt, corres, 0, 1024, rr.MAX_DIST, 3, 0.9, rr.MAX_DIST, 7)
    per = (hy["flags"] == 3).reshape(-1, 32).sum(1)
    assert (per[1:-1] == 0).any() and (per[1:-1] == 1).any() and hy["sens_flags"].sum() == 0
    ref = rr.run(src, tgt, corres, rr.MAX_DIST, 3, 0.9, rr.MAX_DIST, max_iteration=1024, confidence=1.0, seed=7)
    res = _full(r3d, src, tgt, corres, max_iteration=1024, confidence=1.0, seed=7, batch=32)
    _check_against_run(res, ref, src, tgt, corres)
    assert res["validated"] == per.sum()


def test_one_share_and_split_runs_give_the_same_bits(r3d, monkeypatch):
    """M = 2 049 is three summation runs.  By default the few survivors' runs are split over the grid and k_ransac_reduce folds the
    per-run partials; with the partials buffer taken away (R3D_RANSAC_PART_ELEMS=0, a diagnostic switch) every thread folds its
    three runs itself.  Same additions in the same order: count and err2 equal bit for bit, and so does a full run."""
    src, tgt, corres, _, _ = rr.planted_case(2 * rr.RUN + 1, 800, seed=77)
    kw = dict(h0=5, count=700, max_correspondence_distance=rr.MAX_DIST, ransac_n=3, edge_length=None, checker_distance=0.0, seed=3)
    split = r3d.cloud_ops.debug_ransac_hypotheses(src, tgt, corres, **kw)
    full_split = _full(r3d, src, tgt, corres, max_iteration=2000, confidence=1.0)
    monkeypatch.setenv("R3D_RANSAC_PART_ELEMS", "0")
    one = r3d.cloud_ops.debug_ransac_hypotheses(src, tgt, corres, **kw)
    full_one = _full(r3d, src, tgt, corres, max_iteration=2000, confidence=1.0)
    monkeypatch.delenv("R3D_RANSAC_PART_ELEMS")
    assert (split["flags"] == 3).all() and split["inliers"].max() > 0
    for k in ("samples", "flags", "inliers"):
        assert np.array_equal(split[k], one[k])
    assert split["err2"].tobytes() == one["err2"].tobytes() and split["T"].tobytes() == one["T"].tobytes()
    hy = rr.hypotheses(src, tgt, corres, 5, 700, rr.MAX_DIST, 3, None, 0.0, 3)
    ok = ~hy["ill"] & (hy["sens_pairs"] == 0)
    assert np.array_equal(one["inliers"][ok], hy["inliers"][ok])
    assert (np.abs(one["err2"][ok] - hy["err2"][ok]) <= 1e-9 * hy["err2"][ok]).all()
    for k in ("best_hypothesis", "iterations", "validated", "inliers", "inlier_rmse"):
        assert full_split[k] == full_one[k], k
    assert full_split["T"].tobytes() == full_one["T"].tobytes()


def _raw(r3d, fn, prm, s, t, c, m=None, ns=None, nt=None, T=True):
    ctx = r3d.default_context()
    p = lambda a: None if a is None else a.ctypes.data_as(_vp)       # noqa: E731
    out, st = np.empty((4, 4)), r3d.cloud_ops.RansacStats()
    args = [ctypes.byref(prm), p(s), len(s) if ns is None else ns, p(t), len(t) if nt is None else nt, p(c), len(c) if m is None else m]
    if fn == "r3d_debug_ransac_hypotheses":
        args += [0, 16, None, None, None, None, None]
    else:
        args += [p(out) if T else None, None, ctypes.byref(st)]
    with pytest.raises(r3d.R3DError) as e:
        ctx.call(fn, *args)
    return e.value.code


def test_refusals(r3d):
    src, tgt, corres, _, _ = rr.planted_case(600, 220, seed=603)
    P = lambda **kw: r3d.cloud_ops._ransac_params(**{**dict(max_correspondence_distance=0.02, ransac_n=3, edge_length=0.9,       # noqa: E731
                                                          checker_distance=None, max_iteration=1000, confidence=0.999, seed=0, batch=0), **kw})
    BADARG, UNSUPPORTED = -1, -4
    for fn in ("r3d_ransac_correspondence", "r3d_debug_ransac_hypotheses"):
        assert _raw(r3d, fn, P(), None, tgt, corres, ns=600) == BADARG
        assert _raw(r3d, fn, P(), src, None, corres, nt=600) == BADARG
        assert _raw(r3d, fn, P(), src, tgt, None, m=600) == BADARG
        assert _raw(r3d, fn, P(), src, tgt, corres, m=2) == BADARG                       # M < ransac_n
        assert _raw(r3d, fn, P(ransac_n=4), src, tgt, corres, m=3) == BADARG
        assert _raw(r3d, fn, P(max_correspondence_distance=0.0), src, tgt, corres) == BADARG
        assert _raw(r3d, fn, P(confidence=0.0), src, tgt, corres) == BADARG
        assert _raw(r3d, fn, P(max_iteration=0), src, tgt, corres) == BADARG
        assert _raw(r3d, fn, P(ransac_n=2), src, tgt, corres) == UNSUPPORTED
        assert _raw(r3d, fn, P(ransac_n=5), src, tgt, corres) == UNSUPPORTED
        assert _raw(r3d, fn, P(max_iteration=2 ** 31), src, tgt, corres) == UNSUPPORTED
        for row, col, v in ((17, 0, 600), (599, 1, 600), (0, 0, -1), (300, 1, 2 ** 31 - 1)):   # a pair index outside its cloud
            bad = corres.copy()
            bad[row, col] = v
            assert _raw(r3d, fn, P(), src, tgt, bad) == BADARG
    assert _raw(r3d, "r3d_ransac_correspondence", P(), src, tgt, corres, T=False) == BADARG
    ctx = r3d.default_context()
    bad = corres.copy()
    bad[123, 1] = 600
    d_s, d_t, d_c = ctx.to_device(src), ctx.to_device(tgt), ctx.to_device(bad)
    try:
        with pytest.raises(r3d.R3DError) as e:                       # checked on the device, before any hypothesis reads it
            r3d.cloud_ops.registration_ransac_based_on_correspondence_device(d_s, 600, d_t, 600, d_c, 600, 0.02, max_iteration=100)
        assert e.value.code == BADARG and "outside its cloud" in str(e.value)
        with pytest.raises(r3d.R3DError) as e:
            r3d.cloud_ops.registration_ransac_based_on_correspondence_device(d_s, 600, 0, 600, d_c, 600, 0.02)
        assert e.value.code == BADARG
    finally:
        for d in (d_s, d_t, d_c):
            ctx.free(d)
    res = _full(r3d, src, tgt, corres, max_iteration=4096)          # the context works on after the refusals
    assert res["inliers"] == 220


def test_device_form_equals_host_form(r3d):
    src, tgt, corres, _, planted = rr.planted_case(2000, 416, seed=2003)
    ctx = r3d.default_context()
    host = _full(r3d, src, tgt, corres)
    d_s, d_t, d_c, d_m = ctx.to_device(src), ctx.to_device(tgt), ctx.to_device(corres), ctx.alloc(2000)
    try:
        dev = r3d.cloud_ops.registration_ransac_based_on_correspondence_device(d_s, 2000, d_t, 2000, d_c, 2000, rr.MAX_DIST, edge_length=0.9,
                                                                               max_iteration=8192, d_inlier_mask=d_m)
        mask = np.empty(2000, np.uint8)
        ctx.d2h(mask, d_m)
        nomask = r3d.cloud_ops.registration_ransac_based_on_correspondence_device(d_s, 2000, d_t, 2000, d_c, 2000, rr.MAX_DIST,
                                                                                  max_iteration=8192)
    finally:
        for d in (d_s, d_t, d_c, d_m):
            ctx.free(d)
    for r in (dev, nomask):
        for k in ("best_hypothesis", "iterations", "validated", "inliers", "fitness", "inlier_rmse"):
            assert r[k] == host[k], k
        assert r["T"].tobytes() == host["T"].tobytes()
    assert np.array_equal(mask != 0, planted) and np.array_equal(corres[mask != 0], host["correspondence_set"])


# ---- the recorded frame against a moved, thinned copy of itself
def test_feature_matching_wrapper_on_the_recorded_frame(r3d):
    p, nm, q, qn, t_true = rr.frame_pair()
    fs, ft = r3d.compute_fpfh_feature(p, nm, 0.1, 100), r3d.compute_fpfh_feature(q, qn, 0.1, 100)
    corres = r3d.correspondences_from_features(fs, ft, mutual_filter=True)
    kw = dict(ransac_n=3, edge_length=0.9, checker_distance=0.03, max_iteration=100000, confidence=0.999, seed=3)
    res = r3d.registration_ransac_based_on_feature_matching(p, q, fs, ft, True, 0.03, **kw)
    ref = rr.run(p, q, corres, 0.03, 3, 0.9, 0.03, 100000, 0.999, 3, chunk=64)
    d_true = np.sqrt(((p[corres[:, 0]] @ t_true[:3, :3].T + t_true[:3, 3] - q[corres[:, 1]]) ** 2).sum(1))
    print(f"frame pair: {len(corres)} mutual pairs, {(d_true < 0.03).mean():.1%} within 0.03 of the truth; iterations {res['iterations']}, "
          f"validated {res['validated']}, inliers {res['inliers']}, |T - truth| {np.abs(res['T'] - t_true).max():.2e}")
    _check_against_run(res, ref, p, q, corres, 0.03)
    assert len(corres) > 3000 and (d_true < 0.03).mean() > 0.8      # the features find the motion's pairs
    assert np.abs(res["T"] - t_true).max() < 0.03
    # the device form of the wrapper: same searches, same estimator
    ctx = r3d.default_context()
    ptrs = [ctx.to_device(a) for a in (p, q, np.ascontiguousarray(fs.T), np.ascontiguousarray(ft.T))]
    try:
        dev = r3d.cloud_ops.registration_ransac_based_on_feature_matching_device(ptrs[0], len(p), ptrs[1], len(q), ptrs[2], ptrs[3], True, 0.03, **kw)
    finally:
        for d in ptrs:
            ctx.free(d)
    assert dev["T"].tobytes() == res["T"].tobytes() and dev["best_hypothesis"] == res["best_hypothesis"]
    assert np.array_equal(dev["correspondence_set"], res["correspondence_set"])


def test_global_registration_feeds_multi_scale_icp(r3d):
    p, _, q, _, t_true = rr.frame_pair()
    pa = r3d.pointcloud_alignment
    voxel = 0.02
    t0, res = pa.global_registration(p, q, voxel, seed=0, max_iteration=100000)
    assert res["best_hypothesis"] >= 0 and res["inliers"] == len(res["correspondence_set"]) > 0
    sd, td, cs = res["source_down"], res["target_down"], res["correspondence_set"]
    d = np.sqrt(((sd[cs[:, 0]] @ t0[:3, :3].T + t0[:3, 3] - td[cs[:, 1]]) ** 2).sum(1))
    assert (d < 1.5 * voxel + rr.BAND).all()                        # RANSAC's reported inliers are inliers under its T
    t1, scales = pa.multi_scale_icp(sd, td, voxel, init=t0, target_normals=res["target_normals"])
    assert len(scales) == 3 and np.isfinite(t1).all()
    print(f"global_registration: {len(sd)} / {len(td)} points, inliers {res['inliers']}, |T_ransac - truth| {np.abs(t0 - t_true).max():.2e}, "
          f"after multi_scale_icp {np.abs(t1 - t_true).max():.2e}")
