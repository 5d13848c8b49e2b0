"""CPU: tests/icp_step_ref.py (the restatement of one registration step) against oracle/cloud_oracle.py on a benign cloud, and
the conditions every case of tests/icp_step_cases.py must meet for tests/test_icp_step_gpu.py to mean what it says."""
import functools

import numpy as np
import pytest

from oracle import cloud_oracle as co
from tests import icp_step_cases as cs
from tests import icp_step_ref as ref

CASES = {c["name"]: c for c in cs.small_cases()}


@functools.lru_cache(maxsize=None)
def _eval(name, mode):
    c = CASES[name]
    ev = ref.evaluate(c["src"], c["tgt"], c["md"], mode, c["init"], c["sn"], c["tn"], c["eps"])
    return ev, ref.step(ev, mode)


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_one_step_equals_the_oracle_on_the_benign_ellipsoid(mode):
    tgt, tn = cs.ellipsoid(1500, 3)
    Ti = np.linalg.inv(cs.MOTION)
    src = cs.apply(Ti, cs.ellipsoid(1200, 4)[0])
    sn = cs.ellipsoid(1200, 4)[1] @ Ti[:3, :3].T
    init = cs.rigid((0, 0, 1), 0.3, (0.001, 0, 0))
    ev = ref.evaluate(src, tgt, 0.05, mode, init, sn, tn, 1e-3)
    U, info = ref.step(ev, mode)
    want = co.registration(src, tgt, 0.05, init=init, mode=("p2p", "p2plane", "gicp")[mode], max_iteration=1, target_normals=tn,
                           source_cov=co.covariances_from_normals(sn), target_cov=co.covariances_from_normals(tn))
    assert ev["n"] > 1000 and (mode == 0 or info["solved"])
    # the oracle sums in float64: it may lose what step_tolerance allows the device
    assert np.abs(U @ init - want["T"]).max() <= ref.step_tolerance(info, mode, U @ init)
    # the statistics of the oracle's second evaluation are those of an evaluation at the pose it returns
    ev2 = ref.evaluate(src, tgt, 0.05, 0, want["T"])
    assert ev2["n"] == want["correspondences"] and want["fitness"] == ev2["n"] / len(src)
    assert abs(ref.rmse(ev2) - want["inlier_rmse"]) <= ref.rmse_tolerance(ev2)


def test_inverse_and_slot_layout():
    rng = np.random.default_rng(0)
    M = rng.random((5, 3, 3)) + 2 * np.eye(3)
    np.testing.assert_allclose(ref._inv3(M.astype(ref.LD)).astype(float), np.linalg.inv(M), rtol=1e-13)
    assert len(ref.TRIU) == 21 and ref.TRIU[0] == (0, 0) and ref.TRIU[6] == (1, 1) and ref.TRIU[20] == (5, 5)
    # the header's formula gives back the centred covariance from slots relative to any origin
    c = CASES["far_c100"]
    o = c["tgt"].mean(0) + 0.1
    ev = ref.evaluate(c["src"], c["tgt"], c["md"], 0, None, origin=o)
    mp, mt, sigma = ref.p2p_from_slots(ev["value"].astype(float), o)
    bq, bu, bs = ref.p2p_derived_bounds(ev)
    assert (np.abs(mp - ev["mean_p"].astype(float)) <= bq + 1e-13).all() and (np.abs(mt - ev["mean_t"].astype(float)) <= bu + 1e-13).all()
    assert (np.abs(sigma - ev["sigma"].astype(float)) <= bs).all()


def test_sliced_search_is_the_brute_force():
    from tests import neighbor_ref as nr
    s, t, _, _ = cs.sized(20011, 300)
    a, b = ref.nearest(t, s, cs.MOTION, 0.05), nr.brute_nearest(t, s, cs.MOTION, 0.05)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and (a[0] >= 0).sum() > 10000


@pytest.mark.parametrize("name", list(CASES))
def test_six_by_six_determinants_are_far_from_the_rule(name):
    """neither side's rounding can cross |det| < 1e-6: the reference's |det| lies outside [1e-9, 1e-3]"""
    for mode in CASES[name]["modes"]:
        if mode == 0:
            continue
        ev, (U, info) = _eval(name, mode)
        if ev["n"]:
            assert not (1e-9 <= abs(info["det"]) <= 1e-3), (mode, info["det"])
            assert info["solved"] == (abs(info["det"]) >= 1e-6)


def test_chunk_cases_have_the_sizes_that_take_each_branch():
    got = {c["name"]: (len(c["src"]) + cs.ICP_BLOCK - 1) // cs.ICP_BLOCK for c in cs.chunk_cases()}
    assert [got[f"ns{n}"] for n in (1, 63, 64, 65, 255, 256, 257)] == [1, 1, 1, 1, 1, 1, 2]
    assert [got[f"chunks{k}"] for k in (8, 16, 24, 9, 13)] == [8, 16, 24, 9, 13]
    for c in cs.chunk_cases():
        assert len(c["tgt"]) == 500 and _eval(c["name"], 0)[0]["n"] >= 0.9 * len(c["src"])
    big = cs.large_case(256)
    assert len(big["src"]) == (3 * 256 + 1) * 256 + 17 and len(big["tgt"]) == 2000


def test_masked_cases_mask_what_they_say():
    ev = _eval("half_far", 0)[0]
    assert ev["n"] == 300 and (ev["i"] % 2 == 1).all()
    ev = _eval("chunk_of_zeros", 0)[0]
    assert ev["n"] == 300 and (ev["i"] < 300).all() and len(CASES["chunk_of_zeros"]["src"]) == 900
    far = CASES["chunk_of_zeros"]["src"][300:]
    assert (far.max(0) < CASES["chunk_of_zeros"]["tgt"].min(0) - 1.0).all()      # one corner cell of the grid for all 600
    for mode in (0, 1, 2):
        ev, (U, info) = _eval("no_correspondence", mode)
        assert ev["n"] == 0 and np.array_equal(U, np.eye(4)) and ref.rmse(ev) == 0.0


def test_boundary_pair_is_exactly_at_the_distance():
    a, b = _eval("at_distance", 0)[0], _eval("one_ulp_inside", 0)[0]
    c = CASES["at_distance"]
    d = c["src"][0] - c["tgt"][0]
    assert float(d @ d) == c["md"] ** 2 == 0.0625
    assert a["n"] == 4 and 0 not in a["i"] and b["n"] == 5 and b["i"][0] == 0 and b["j"][0] == 0
    assert b["d2"][0] < 0.0625 and np.nextafter(CASES["one_ulp_inside"]["src"][0, 0], 1.0) == 0.25


def test_few_pair_cases_have_the_ranks_they_name():
    want = dict(pairs1=0, pairs2=1, pairs3=2, pairs4=3, pairs5=3, collinear6=1)
    for name, rank in want.items():
        ev, (U, info) = _eval(name, 0)
        assert ev["n"] == len(CASES[name]["src"]) and info["rank"] == rank, name
        assert not _eval(name, 1)[1][1]["solved"], name                       # fewer than six rows: singular
    for name in ("pairs1", "pairs2", "collinear6"):
        assert not _eval(name, 2)[1][1]["solved"], name
    assert not _eval("parallel_normals", 1)[1][1]["solved"] and _eval("parallel_normals", 2)[1][1]["solved"]


def test_flat_cases_are_flat():
    for c in cs.flat_cases():
        ev, (U, info) = _eval(c["name"], 0)
        th = float(c["name"].split("_")[1][2:])
        assert ev["n"] == 300 and len(c["tgt"]) == 300
        assert info["rank"] == (3 if th >= 1e-2 else 2), (c["name"], info["sv"])
        assert info["sv"][1] > 0.1 * info["sv"][0]                              # two directions of the patch's extent
        assert np.isfinite(ref.step_tolerance(info, 0, U))
    assert len(cs.flat_cases()) == 5 * 3 * 2


def test_far_cases_move_about_their_own_centre():
    for c, off in zip(cs.far_cases(), cs.OFFSETS):
        centre = off * np.array([1.0, -0.6, 0.8])
        assert np.abs(c["tgt"].mean(0) - centre).max() < 0.05 and len(c["src"]) == 1000
        for mode in (0, 1, 2):
            ev, (U, info) = _eval(c["name"], mode)
            assert ev["n"] == 1000
            assert np.abs(U[:3, :3] - cs.MOTION[:3, :3]).max() < 5e-3            # a step towards that degree, at every offset
            if mode == 0:      # (the absolute p x n of the plane modes loses this at the far offsets: cond(J^T J) ~ 1e15)
                assert np.linalg.norm(U[:3, :3] @ centre + U[:3, 3] - centre) < 0.05


def test_gicp_cases_hold_the_quirk_and_zero_normals_among_their_pairs():
    for c in cs.gicp_cases():
        ev, (U, info) = _eval(c["name"], 2)
        assert ev["n"] == 300 and info["solved"]
        both = [0, 1, 2, 30, 31, 32, 33]                                         # pairs whose two normals are the special ones
        assert (ev["j"][both] == both).all() and np.isin(np.arange(10, 14), ev["j"]).all()
        for k, nx in enumerate(cs.QUIRK_NX):
            assert c["tn"][10 + k, 0] == nx and c["sn"][20 + k, 0] == nx and c["tn"][30 + k, 0] == c["sn"][30 + k, 0] == nx
        assert (ref.effective_normals(c["tn"][10:14])[:, 0] == [1.0, 1.0, -0.99, -0.985]).all()   # the rule is a strict <
        assert not c["tn"][0:3].any() and not c["sn"][0:3].any()                 # both normals zero: M = 2 I
    eps0, eps3 = _eval("gicp_eps0_init0", 2)[0], _eval("gicp_eps0.001_init0", 2)[0]
    assert np.array_equal(eps0["value"], eps3["value"])                          # epsilon 0 selects 1e-3
    init = CASES["gicp_eps0.001_init40"]["init"]
    assert np.degrees(np.arccos((np.trace(init[:3, :3]) - 1) / 2)) == pytest.approx(40.0)
