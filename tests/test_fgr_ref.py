"""CPU tests of the numpy restatement of Fast Global Registration (tests/fgr_ref.py): its two forms agree, it reproduces the
figures recorded with the contract ("FGR"), and the cases tests/test_fgr_gpu.py compares are fit to be
compared: no trial near a threshold before the cut, no transform that moves when the rows are summed in another order."""
import numpy as np
import pytest

from tests import fgr_ref as fr
from tests import ransac_ref as rr


def _run(name, **kw):
    src, tgt, corres, t_true, is_planted = fr.planted(name)
    return fr.run(src, tgt, corres, seed=fr.TRIAL_SEED, **kw), (src, tgt, corres, t_true, is_planted)


def test_literal_and_vectorised_forms_agree():
    src, tgt, corres, _, _ = fr.planted("planted257")
    a = fr.run(src, tgt, corres, seed=fr.TRIAL_SEED)
    b = fr.run(src, tgt, corres, seed=fr.TRIAL_SEED, literal=True)
    assert (a["tuples"], a["trials"], a["pairs"]) == (b["tuples"], b["trials"], b["pairs"])
    assert np.array_equal(a["index"], b["index"])
    assert np.abs(a["rows"] - b["rows"]).max() <= 1e-15
    assert np.abs(a["trace_T"] - b["trace_T"]).max() <= 1e-15
    assert np.array_equal(a["trace_par"], b["trace_par"])
    assert np.abs(a["T"] - b["T"]).max() <= 1e-15
    # and on a few trials of every tuple case, flag by flag
    for name, (ncorr, t0, count, scale) in fr.TUPLE_CASES.items():
        s, t, c = fr.pairs_case(ncorr)
        sn, tn, _ = fr.normalise(s, t)
        p, q = sn[c[:, 0]], tn[c[:, 1]]
        n = min(count, 200)
        smp, flags, _ = fr.tuple_trials(p, q, t0, n, scale, fr.TRIAL_SEED)
        for i in range(n):
            ci, fi = fr.tuple_trial_literal(p, q, t0 + i, scale, fr.TRIAL_SEED)
            assert ci == smp[i].tolist() and fi == flags[i], (name, i)


@pytest.mark.parametrize("name", sorted(fr.PLANTED))
def test_planted_cases_give_the_recorded_figures(name):
    res, (src, tgt, corres, t_true, is_planted) = _run(name)
    accepted, cut_trial = fr.PLANTED_EXPECT[name]
    # the accepted trials of all 100 ncorr, without the cut
    sn, tn, _ = fr.normalise(src, tgt)
    _, flags, sens = fr.tuple_trials(sn[corres[:, 0]], tn[corres[:, 1]], 0, fr.TRIALS_PER_PAIR * len(corres), 0.95, fr.TRIAL_SEED)
    assert int(flags.sum()) == accepted
    if cut_trial is None:
        assert res["tuples"] == accepted and res["trials"] == fr.TRIALS_PER_PAIR * len(corres)
    else:
        assert res["tuples"] == 1000 and res["trials"] == cut_trial + 1 and flags[cut_trial] == 1
    assert res["pairs"] == 3 * res["tuples"]
    # par takes eleven divisions and holds from iteration 40
    par = 1.0
    for _ in range(11):
        par /= 1.4
    assert res["final_par"] == par and abs(par - 0.0246940093) < 1e-10
    assert (res["trace_par"][40:] == par).all() and res["trace_par"][39] > par
    # the planted points land within the noise amplitude of the truth
    moved = src[corres[is_planted, 0]] @ res["T"][:3, :3].T + res["T"][:3, 3]
    truth = src[corres[is_planted, 0]] @ t_true[:3, :3].T + t_true[:3, 3]
    err = np.abs(moved - truth).max()
    print(f"{name}: {res['tuples']} tuples of {accepted} accepted, {res['trials']} trials, {is_planted[res['index']].mean():.0%} of the rows "
          f"planted, max error on planted points {err:.2e}")
    assert err < 0.002
    assert not res["failed"]


@pytest.mark.parametrize("name", sorted(fr.PLANTED))
def test_parity_cases_have_no_trial_near_a_threshold(name):
    res, _ = _run(name)
    assert res["sensitive"] == 0
    # the case that puts the cut on a batch edge shares these trials: its cut lies before this one


@pytest.mark.parametrize("name", sorted(fr.TUPLE_CASES))
def test_tuple_cases_report_their_sensitive_trials(name):
    ncorr, t0, count, scale = fr.TUPLE_CASES[name]
    s, t, c = fr.pairs_case(ncorr)
    sn, tn, _ = fr.normalise(s, t)
    smp, flags, sens = fr.tuple_trials(sn[c[:, 0]], tn[c[:, 1]], t0, count, scale, fr.TRIAL_SEED)
    assert smp.shape == (count, 3) and smp.min() >= 0 and smp.max() < ncorr
    assert sens.sum() <= count // 100                                # the loose ones stay rare (tuple_scale 1.0: ties excluded below)
    if scale == 1.0:
        assert flags.sum() == 0
    if ncorr == 1:
        assert flags.sum() == 0 and sens.sum() == 0                  # every edge is 0 < 0


@pytest.mark.parametrize("name", sorted(fr.PLANTED))
def test_reverse_order_summation_moves_no_transform(name):
    res, _ = _run(name)
    _, _, fwd, _, _ = fr.optimise(res["rows"], 1.0, 0.025)
    _, _, rev, _, _ = fr.optimise(res["rows"], 1.0, 0.025, reverse=True)
    moved = np.abs(fwd - rev).max()
    print(f"{name}: reverse-order summation moves the 64 transforms by at most {moved:.1e}")
    assert moved <= 1e-14


@pytest.mark.parametrize("m,kw", fr.TRACE_CASES, ids=fr.TRACE_IDS)
def test_trace_cases_are_well_conditioned(m, kw):
    kw = dict(kw)
    src, tgt, corres = fr.trace_case(m, grid=kw.pop("grid", False), big=kw.pop("big", "source"))
    o = fr.options(**kw)
    assert len(corres) == m and len(src) != len(tgt)
    sn, tn, nrm = fr.normalise(src, tgt, o["use_absolute_scale"])
    rows = np.concatenate([sn[corres[:, 0]], tn[corres[:, 1]]], 1)
    args = (rows, nrm["scale_start"], o["maximum_correspondence_distance"], o["division_factor"], o["iteration_number"], o["decrease_mu"])
    _, _, fwd, _, failed = fr.optimise(*args)
    _, _, rev, _, _ = fr.optimise(*args, reverse=True)
    assert not failed
    assert np.abs(fwd - rev).max(initial=0.0) <= 1e-14
    # the largest norm lies where the case says, and a grid case has exact means whatever the order
    for big in ("source", "target"):
        s, t, _ = fr.trace_case(m, grid=True, big=big)
        cs, ct = s - s.mean(0), t - t.mean(0)
        assert (np.linalg.norm(cs, axis=1).max() > np.linalg.norm(ct, axis=1).max()) == (big == "source")
        for c in (s, t):
            assert np.array_equal(np.add.reduce(c, 0), np.add.reduce(c[::-1], 0))


def test_few_pairs_quirk_and_solve_failure_rule(monkeypatch):
    src, tgt, corres, _, _ = fr.planted("planted257")
    res = fr.run(src, tgt, corres[:9], tuple_test=False)
    assert res["pairs"] == 9 and len(res["trace_T"]) == 0 and np.array_equal(res["trans"], np.eye(4))
    want = np.eye(4)
    want[:3, 3] = tgt.mean(0) - src.mean(0)
    assert np.abs(res["T"] - want).max() < 1e-15                     # QUIRK_FEW_PAIRS: centroid to centroid, not the identity
    monkeypatch.setattr(fr, "QUIRK_FEW_PAIRS", False)
    assert np.array_equal(fr.run(src, tgt, corres[:9], tuple_test=False)["T"], np.eye(4))
    monkeypatch.undo()
    # ten pairs run the loop
    assert len(fr.run(src, tgt, corres[:10], tuple_test=False)["trace_T"]) == 64
    # a zero pivot or a non-finite solution gives the identity delta and the loop goes on
    assert fr.ldlt_solve(np.zeros((6, 6)), np.ones(6)) is None
    assert fr.ldlt_solve(np.diag([1.0, 1, 1, 1, 1, np.nan]), np.ones(6)) is None
    assert fr.ldlt_solve(np.diag([1e-300] * 6), np.full(6, 1e300)) is None     # overflows: non-finite x
    a = np.diag([1e-8, 2.0, 3.0, 4.0, 5.0, 6.0])                               # |det| = 7.2e-6 ... 1e-6 apart: no determinant rule here
    assert np.allclose(fr.ldlt_solve(a * 1e-3, np.ones(6)), 1.0 / np.diag(a * 1e-3))
    rows = np.zeros((12, 6))                                                   # every residual and every q zero: JTJ = diag(0, 0, 0, n, n, n)
    trans, par, tr_t, tr_p, failed = fr.optimise(rows, 1.0, 0.025)
    assert failed == list(range(64)) and np.array_equal(trans, np.eye(4)) and tr_p[-1] == par


def test_unscaled_distance_quirk(monkeypatch):
    src, tgt, corres, _, _ = fr.planted("planted257")
    a = fr.run(src, tgt, corres, seed=fr.TRIAL_SEED, maximum_correspondence_distance=0.03)
    monkeypatch.setattr(fr, "QUIRK_UNSCALED_DISTANCE", False)
    b = fr.run(src, tgt, corres, seed=fr.TRIAL_SEED, maximum_correspondence_distance=0.03)
    # scale_global is 0.79 here: 0.03 in normalised units is 0.038, above 1.4^-10 = 0.0346, and the annealing stops a step earlier
    assert a["scale_global"] < 1 and b["final_par"] > a["final_par"]
    assert abs(b["final_par"] - 1.4 ** -10) < 1e-12 and abs(a["final_par"] - 1.4 ** -11) < 1e-12


def test_mutual_pairs_is_the_plain_cross_check():
    nn_st, nn_ts = np.array([2, 0, 0, 1]), np.array([1, 3, 0])
    assert fr.mutual_pairs(nn_st, nn_ts).tolist() == [[0, 2], [1, 0], [3, 1]]
    assert rr.sample_index(7, 0, 0, 600) == int(rr.samples(7, 0, 1, 3, 600)[0, 0])
