"""GPU tests of Fast Global Registration (r3d_fgr_correspondence, r3d_fgr_feature_matching, their _dev forms, r3d_debug_fgr_tuples,
r3d_debug_fgr_optimize and the Python functions over them) against the numpy restatement in tests/fgr_ref.py.

Bars.  The tuple sampler is integer arithmetic: samples are exact.  A trial's flag is exact unless one of its six comparisons
lies within BAND = 1e-12 relative of its threshold (the device's means are two-level sums, the restatement's plain ones: the
normalised coordinates differ in their last bits); tests/test_fgr_ref.py checks that the full-run cases have no such trial before
their cut, so their tuples, trials and pairs are exact.  The annealing parameter is a scalar division chain: bit-equal.  The
transforms (every iteration of the trace, and the result) agree to 1e-12 per entry: the restatement alone moves by 8e-16 when its
rows are summed in reverse order, the device adds its own summation order and sincos; 1e-12 leaves three decades over that and is
nine decades under the 6e-4 the estimator achieves.  Results are byte-identical across batch sizes, across runs and between the
host and device forms.

Measured on the MI355X (the tests print every figure): no flag differs from the restatement on any of the eleven tuple cases
(none has a trial inside the band); max |T - restatement| 6.7e-16 over the four full runs, 1.0e-15 over the twelve optimisation
traces (largest at M = 3000 with use_absolute_scale), 4.4e-16 on the recorded frame pair, where FGR ends 1.5e-4 from the truth
(the restatement: the same 1.5e-4; the bound is the RANSAC test's 0.03 on that pair) with 6002 mutual pairs, 1000 tuples after
1180 trials."""
import ctypes
import functools

import numpy as np
import pytest

from tests import fgr_ref as fr
from tests import ransac_ref as rr

pytestmark = pytest.mark.gpu
BADARG, UNSUPPORTED = -1, -4
BAR = 1e-12


# ---------------------------------------------------------------------------------------------------------------------- tuples
@pytest.mark.parametrize("name", sorted(fr.TUPLE_CASES))
def test_tuple_trials_match_the_restatement(r3d, name):
    ncorr, t0, count, scale = fr.TUPLE_CASES[name]
    src, tgt, corres = fr.pairs_case(ncorr)
    sn, tn, _ = fr.normalise(src, tgt)
    smp, flags, sens = fr.tuple_trials(sn[corres[:, 0]], tn[corres[:, 1]], t0, count, scale, fr.TRIAL_SEED)
    got = r3d.cloud_ops.debug_fgr_tuples(src, tgt, corres, t0, count, tuple_scale=scale, seed=fr.TRIAL_SEED)
    assert np.array_equal(got["samples"], smp)
    assert np.array_equal(got["flags"][~sens], flags[~sens])
    assert set(np.unique(got["flags"])) <= {0, 1}
    print(f"{name}: {count} trials, {int(flags.sum())} accepted, {int(sens.sum())} within the band, "
          f"{int((got['flags'] != flags).sum())} flags differ")
    if scale == 1.0 or ncorr == 1:
        assert got["flags"].sum() == 0


# -------------------------------------------------------------------------------------------- full run, correspondence form
@functools.lru_cache(maxsize=None)
def _full_ref(name):
    if name == "batch_edge":                                         # the cut fills its last place with the last accept of a 1000-trial batch
        src, tgt, corres, _, _ = fr.planted("planted600")
        sn, tn, _ = fr.normalise(src, tgt)
        _, flags, _ = fr.tuple_trials(sn[corres[:, 0]], tn[corres[:, 1]], 0, 1000, 0.95, fr.TRIAL_SEED)
        kw = dict(maximum_tuple_count=int(flags.sum()))
    else:
        src, tgt, corres, _, _ = fr.planted(name)
        kw = {}
    return src, tgt, corres, kw, fr.run(src, tgt, corres, seed=fr.TRIAL_SEED, **kw)


@pytest.mark.parametrize("name", sorted(fr.PLANTED) + ["batch_edge"])
def test_full_run_matches_the_restatement_whatever_the_batch(r3d, name):
    src, tgt, corres, kw, ref = _full_ref(name)
    assert ref["sensitive"] == 0 and ref["pairs"] >= fr.MIN_PAIRS
    runs = [r3d.registration_fgr_based_on_correspondence(src, tgt, corres, seed=fr.TRIAL_SEED, batch=b, **kw) for b in (0, 64, 1000, 0)]
    for res in runs:
        assert (res["matched"], res["tuples"], res["trials"], res["pairs"]) == (len(corres), ref["tuples"], ref["trials"], ref["pairs"])
        assert res["final_par"] == ref["final_par"]
        assert res["T"].tobytes() == runs[0]["T"].tobytes()
        assert (res["fitness"], res["inlier_rmse"], res["correspondences"]) == (runs[0]["fitness"], runs[0]["inlier_rmse"], runs[0]["correspondences"])
    err = np.abs(runs[0]["T"] - ref["T"]).max()
    print(f"{name}: tuples {ref['tuples']}, trials {ref['trials']}, rows {ref['pairs']}; max |T - restatement| {err:.2e}; "
          f"fitness {runs[0]['fitness']:.3f}, rmse {runs[0]['inlier_rmse']:.2e}")
    assert err < BAR
    if name == "batch_edge":
        assert ref["trials"] <= 1000 and ref["tuples"] == kw["maximum_tuple_count"]
    # the evaluation is the registration loop's at that pose
    ev = r3d.cloud_ops.registration(src, tgt, 0.025, init=runs[0]["T"], max_iteration=0)
    assert (ev["fitness"], ev["inlier_rmse"], ev["correspondences"]) == (runs[0]["fitness"], runs[0]["inlier_rmse"], runs[0]["correspondences"])
    assert ev["T"].tobytes() == runs[0]["T"].tobytes()
    assert len(runs[0]["correspondence_set"]) == runs[0]["correspondences"]


# ------------------------------------------------------------------------------------------------------- optimisation trace
def _trace_ref(src, tgt, corres, **kw):
    o = fr.options(**kw)
    sn, tn, nrm = fr.normalise(src, tgt, o["use_absolute_scale"])
    rows = np.concatenate([sn[corres[:, 0]], tn[corres[:, 1]]], 1)
    _, _, tr_t, tr_p, failed = fr.optimise(rows, nrm["scale_start"], o["maximum_correspondence_distance"], o["division_factor"],
                                           o["iteration_number"], o["decrease_mu"], nrm["scale_global"])
    if len(rows) < fr.MIN_PAIRS:                                     # the loop does not run: the device reports the start state
        tr_t = np.broadcast_to(np.eye(4), (o["iteration_number"], 4, 4))
        tr_p = np.full(o["iteration_number"], nrm["scale_start"])
    return tr_t, tr_p, failed, nrm


@pytest.mark.parametrize("m,kw", fr.TRACE_CASES, ids=fr.TRACE_IDS)
def test_optimisation_trace_matches_the_restatement(r3d, m, kw):
    kw = dict(kw)
    src, tgt, corres = fr.trace_case(m, grid=kw.pop("grid", False), big=kw.pop("big", "source"))
    assert len(src) != len(tgt)
    tr_t, tr_p, failed, nrm = _trace_ref(src, tgt, corres, **kw)
    got = r3d.cloud_ops.debug_fgr_optimize(src, tgt, corres, **kw)
    it = fr.options(**kw)["iteration_number"]
    assert got["trace_T"].shape == (it, 4, 4) and got["trace_par"].shape == (it,)
    assert not failed
    assert got["trace_par"].tobytes() == np.ascontiguousarray(tr_p).tobytes()
    err = np.abs(got["trace_T"] - tr_t).max(initial=0.0)
    print(f"M = {m} {kw}: scale_start {nrm['scale_start']!r}, max |trace_T - restatement| over {it} iterations {err:.2e}")
    assert err < BAR
    if m < fr.MIN_PAIRS:
        assert (got["trace_T"] == np.eye(4)).all()


# ------------------------------------------------------------------------------------------------------------- degenerate inputs
def test_pairs_on_one_line_stay_finite_and_orthonormal(r3d):
    rng = np.random.default_rng(11)
    s = np.outer(rng.uniform(-1, 1, 50), [1.0, 2.0, -0.5]) + [0.2, 0.1, 0.3]
    t = s @ rr.rotation([0, 0, 1], 0.4).T + [0.1, 0.0, -0.2]
    corres = np.stack([np.arange(50), np.arange(50)], 1).astype(np.int32)
    for tuple_test in (False, True):
        res = r3d.registration_fgr_based_on_correspondence(s, t, corres, tuple_test=tuple_test, seed=1)
        assert np.isfinite(res["T"]).all() and np.isfinite([res["fitness"], res["inlier_rmse"], res["final_par"]]).all()
        r = res["T"][:3, :3]
        assert np.abs(r @ r.T - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(r) - 1) < 1e-12
        assert (res["T"][3] == [0, 0, 0, 1]).all()


def test_fewer_than_ten_rows_give_the_centroid_translation(r3d):
    src, tgt, corres, _, _ = fr.planted("planted257")
    for rows in (corres[:9], corres[:1]):
        res = r3d.registration_fgr_based_on_correspondence(src, tgt, rows, tuple_test=False)
        ref = fr.run(src, tgt, rows, tuple_test=False)
        assert res["pairs"] == len(rows) and res["tuples"] == 0 and res["trials"] == 0 and res["final_par"] == 1.0
        assert np.abs(res["T"] - ref["T"]).max() < BAR and (res["T"][:3, :3] == np.eye(3)).all()
        assert np.abs(res["T"][:3, 3] - (tgt.mean(0) - src.mean(0))).max() < BAR
    # three pairs through the tuple test: 300 trials, too few rows whatever they accept
    res = r3d.registration_fgr_based_on_correspondence(src, tgt, corres[:3], seed=fr.TRIAL_SEED)
    ref = fr.run(src, tgt, corres[:3], seed=fr.TRIAL_SEED)
    assert (res["tuples"], res["trials"], res["pairs"]) == (ref["tuples"], ref["trials"], ref["pairs"]) and res["trials"] == 300


def test_refusals(r3d):
    co = r3d.cloud_ops
    src, tgt, corres, _, _ = fr.planted("planted257")

    def refused(code, fn, *a, **k):
        with pytest.raises(r3d.R3DError) as e:
            fn(*a, **k)
        assert e.value.code == code, str(e.value)
        return str(e.value)

    f = r3d.registration_fgr_based_on_correspondence
    for bad in (dict(division_factor=1.0), dict(maximum_correspondence_distance=0.0), dict(tuple_scale=0.0), dict(tuple_scale=1.5),
                dict(iteration_number=-1), dict(maximum_tuple_count=0), dict(batch=-1), dict(division_factor=float("nan"))):
        refused(BADARG, f, src, tgt, corres, **bad)
    refused(BADARG, f, np.zeros((0, 3)), tgt, corres)                # ns < 1
    refused(BADARG, f, src, np.zeros((0, 3)), corres)
    for rows in (np.array([[0, 257]], np.int32), np.array([[-1, 0]], np.int32), np.array([[257, 0]], np.int32)):
        assert "outside its cloud" in refused(BADARG, f, src, tgt, np.concatenate([corres, rows]))
    refused(BADARG, f, np.ones((20, 3)), np.ones((30, 3)), corres[:5] % 20)      # clouds without extent: scale == 0
    refused(BADARG, co.debug_fgr_tuples, src, tgt, corres, 0, 0)
    refused(BADARG, co.debug_fgr_tuples, src, tgt, corres, 0, 262145)
    refused(BADARG, co.debug_fgr_tuples, src, tgt, corres, -1, 4)
    ctx = r3d.default_context()
    d_s, d_t, d_c = ctx.to_device(src), ctx.to_device(tgt), ctx.to_device(np.concatenate([corres, [[0, 257]]]).astype(np.int32))
    feat = ctx.to_device(np.zeros((257, 33)))
    vp = ctypes.c_void_p
    try:
        dev = co.registration_fgr_based_on_correspondence_device
        assert "outside its cloud" in refused(BADARG, dev, d_s, 257, d_t, 257, d_c, 258)       # checked on the device before any read
        refused(BADARG, dev, 0, 257, d_t, 257, d_c, 257)                                       # a missing array
        refused(BADARG, dev, d_s, 257, d_t, 257, 0, 257)
        refused(BADARG, dev, d_s, 0, d_t, 257, d_c, 257)
        refused(UNSUPPORTED, dev, d_s, 2 ** 31, d_t, 257, d_c, 257)                            # counts above 2^31 - 1: refused before any read
        refused(UNSUPPORTED, dev, d_s, 257, d_t, 257, d_c, 2 ** 31)
        fdev = co.registration_fgr_based_on_feature_matching_device
        refused(BADARG, fdev, d_s, 257, d_t, 257, 0, feat)
        refused(UNSUPPORTED, fdev, d_s, 2 ** 31, d_t, 257, feat, feat)
        prm, T, st = co._fgr_params(), np.empty((4, 4)), co.FgrStats()
        with pytest.raises(r3d.R3DError) as e:                                                 # dim != 33
            ctx.call("r3d_fgr_feature_matching_dev", ctypes.byref(prm), vp(d_s), 257, vp(d_t), 257, vp(feat), vp(feat), 32, T.ctypes.data_as(vp),
                     ctypes.byref(st))
        assert e.value.code == UNSUPPORTED
        with pytest.raises(r3d.R3DError) as e:                                                 # a size r3d_match_features refuses
            ctx.call("r3d_fgr_feature_matching_dev", ctypes.byref(prm), vp(d_s), 2 ** 30, vp(d_t), 2 ** 30, vp(feat), vp(feat), 33,
                     T.ctypes.data_as(vp), ctypes.byref(st))
        assert e.value.code == UNSUPPORTED
    finally:
        for d in (d_s, d_t, d_c, feat):
            ctx.free(d)
    res = f(src, tgt, corres, seed=fr.TRIAL_SEED)                    # the context works on after the refusals
    assert res["tuples"] == 39


# ------------------------------------------------------------------------------------------------------------------ device forms
def test_device_correspondence_form_equals_host_form(r3d):
    src, tgt, corres, kw, ref = _full_ref("planted2000")
    host = r3d.registration_fgr_based_on_correspondence(src, tgt, corres, seed=fr.TRIAL_SEED)
    ctx = r3d.default_context()
    ptrs = [ctx.to_device(a) for a in (src, tgt, corres)]
    try:
        dev = r3d.cloud_ops.registration_fgr_based_on_correspondence_device(ptrs[0], len(src), ptrs[1], len(tgt), ptrs[2], len(corres),
                                                                            seed=fr.TRIAL_SEED)
    finally:
        for d in ptrs:
            ctx.free(d)
    assert dev["T"].tobytes() == host["T"].tobytes()
    for k in ("fitness", "inlier_rmse", "correspondences", "matched", "trials", "tuples", "pairs", "scale_global", "scale_start", "final_par"):
        assert dev[k] == host[k], k


# ------------------------------------------------------------------------------------------------------------------ feature form
_FRAME = {}


def _frame(r3d):
    if not _FRAME:
        p, nm, q, qn, t_true = rr.frame_pair()
        fs, ft = r3d.compute_fpfh_feature(p, nm, 0.1, 100), r3d.compute_fpfh_feature(q, qn, 0.1, 100)
        _FRAME.update(p=p, q=q, fs=fs, ft=ft, t_true=t_true)
    return _FRAME


def test_feature_form_on_the_recorded_frame(r3d):
    fx = _frame(r3d)
    p, q, fs, ft, t_true = fx["p"], fx["q"], fx["fs"], fx["ft"], fx["t_true"]
    nn_st, _ = r3d.cloud_ops.match_features(fs, ft, False)
    nn_ts, _ = r3d.cloud_ops.match_features(ft, fs, False)
    mutual = fr.mutual_pairs(nn_st, nn_ts)
    res = r3d.registration_fgr_based_on_feature_matching(p, q, fs, ft, seed=3)
    assert res["matched"] == len(mutual)
    ref = fr.run(p, q, mutual, seed=3)
    err_ref, err_dev = np.abs(ref["T"] - t_true).max(), np.abs(res["T"] - t_true).max()
    print(f"frame pair: {len(p)} / {len(q)} points, {len(mutual)} mutual pairs; tuples {res['tuples']} (restatement {ref['tuples']}), trials "
          f"{res['trials']} ({ref['trials']}), {ref['sensitive']} trials within the band; |T - truth| {err_dev:.2e} (restatement {err_ref:.2e}); "
          f"|T - restatement| {np.abs(res['T'] - ref['T']).max():.2e}; fitness {res['fitness']:.3f}, rmse {res['inlier_rmse']:.2e}")
    # the same pairs through the correspondence form: the same bytes
    corr = r3d.registration_fgr_based_on_correspondence(p, q, mutual, seed=3)
    assert corr["T"].tobytes() == res["T"].tobytes() and (corr["tuples"], corr["trials"]) == (res["tuples"], res["trials"])
    if ref["sensitive"] == 0:
        assert (res["tuples"], res["trials"], res["pairs"]) == (ref["tuples"], ref["trials"], ref["pairs"])
        assert np.abs(res["T"] - ref["T"]).max() < BAR
    assert err_dev < 0.03                                            # the RANSAC test's bound on the same pair
    # the device form: same searches, same estimator, nothing copied to the host
    ctx = r3d.default_context()
    ptrs = [ctx.to_device(a) for a in (p, q, np.ascontiguousarray(fs.T), np.ascontiguousarray(ft.T))]
    try:
        dev = r3d.cloud_ops.registration_fgr_based_on_feature_matching_device(ptrs[0], len(p), ptrs[1], len(q), ptrs[2], ptrs[3], seed=3)
    finally:
        for d in ptrs:
            ctx.free(d)
    assert dev["T"].tobytes() == res["T"].tobytes()
    for k in ("fitness", "inlier_rmse", "correspondences", "matched", "trials", "tuples", "pairs", "final_par"):
        assert dev[k] == res[k], k


def test_global_registration_method_keyword(r3d):
    p, _, q, _, t_true = rr.frame_pair()
    pa = r3d.pointcloud_alignment
    voxel = 0.02
    t0, res = pa.global_registration(p, q, voxel, seed=0, method="fgr")
    assert np.isfinite(t0).all() and res["pairs"] >= fr.MIN_PAIRS and "source_down" in res
    t1, scales = pa.multi_scale_icp(res["source_down"], res["target_down"], voxel, init=t0, target_normals=res["target_normals"])
    assert len(scales) == 3 and np.isfinite(t1).all()
    print(f"global_registration(method='fgr'): {len(res['source_down'])} / {len(res['target_down'])} points, {res['matched']} mutual pairs, "
          f"{res['tuples']} tuples, |T_fgr - truth| {np.abs(t0 - t_true).max():.2e}, after multi_scale_icp {np.abs(t1 - t_true).max():.2e}")
    a, ra = pa.global_registration(p, q, voxel, seed=0, max_iteration=100000)
    b, rb = pa.global_registration(p, q, voxel, seed=0, max_iteration=100000, method="ransac")
    assert a.tobytes() == b.tobytes() and ra["best_hypothesis"] == rb["best_hypothesis"]
    assert np.array_equal(ra["correspondence_set"], rb["correspondence_set"])
    with pytest.raises(ValueError):
        pa.global_registration(p, q, voxel, method="teaser")
