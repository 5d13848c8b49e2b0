"""CPU: mode 3 of tests/icp_step_ref.py (the coloured step) against the restatement of tests/colored_icp_ref.py, and the
conditions every case of tests/colored_step_cases.py must meet for tests/test_colored_step_gpu.py to mean what it says.  The
target records here are the float64 restatement's (tests/colored_icp_ref.color_gradients); on the device they are the device's."""
import functools

import numpy as np
import pytest

from tests import colored_icp_ref as cr
from tests import colored_step_cases as cc
from tests import icp_step_cases as cs
from tests import icp_step_ref as ref

CASES = {c["name"]: c for c in cc.small_cases()}


@functools.lru_cache(maxsize=None)
def _records(name):
    c = CASES[name]
    radius, nn = cc.gradient_setup(c)
    inten, grad, cnt = cr.color_gradients(c["tgt"], c["tn"], c["tc"], radius, nn)
    return np.column_stack([inten, grad]), cnt


@functools.lru_cache(maxsize=None)
def _eval(name):
    c = CASES[name]
    colors = dict(src_intensity=cr.intensity(c["sc"]), tgt_records=_records(name)[0], lambda_geometric=c["lam"])
    ev = ref.evaluate(c["src"], c["tgt"], c["md"], ref.COLORED, c["init"], None, c["tn"], colors=colors)
    return ev, ref.step(ev, ref.COLORED)


def _float64_slots(c, ev, records):
    """the 27 sums in plain float64, from the formulas as tests/colored_icp_ref.compute_transformation writes them"""
    sg, sp = np.sqrt(c["lam"]), np.sqrt(1.0 - c["lam"])
    s, t, nt = ev["p"], ev["t"], c["tn"][ev["j"]]
    it, dt, i_s = records[ev["j"], 0], records[ev["j"], 1:], cr.intensity(c["sc"])[ev["i"]]
    e = ((s - t) * nt).sum(1)
    J_g = sg * np.concatenate([np.cross(s, nt), nt], 1)
    s1 = s - e[:, None] * nt
    i0 = (dt * (s1 - t)).sum(1) + it
    m = -(dt - (dt * nt).sum(1)[:, None] * nt)
    J_i = sp * np.concatenate([np.cross(s, m), m], 1)
    JTJ = J_g.T @ J_g + J_i.T @ J_i
    JTr = J_g.T @ (sg * e) + J_i.T @ (sp * (i_s - i0))
    return np.concatenate([[JTJ[a, b] for a, b in ref.TRIU], JTr])


def test_the_step_equals_the_restatement_of_the_loop():
    """the update of mode 3 against compute_transformation of tests/colored_icp_ref.py, which sums in float64"""
    c = CASES["lambda0.968"]
    ev, (U, info) = _eval(c["name"])
    rec = _records(c["name"])[0]
    want = cr.compute_transformation(ev["p"], ev["t"], c["tn"][ev["j"]], rec[ev["j"], 1:], rec[ev["j"], 0], cr.intensity(c["sc"])[ev["i"]], c["lam"])
    assert ev["n"] > 500 and info["solved"]
    assert np.abs(U - want).max() <= ref.step_tolerance(info, ref.COLORED, U)


@pytest.mark.parametrize("name", list(CASES))
def test_float64_evaluation_is_within_the_bound(name):
    """the plain float64 evaluation of the header's formulas meets the bound the device is held to (at most 8 % of it, on the
    one-pair case, when this was written), and both rows are present in the absolute sums"""
    c = CASES[name]
    ev, _ = _eval(name)
    if ev["n"] == 0:
        assert not ev["value"][1:].any()
        return
    got = _float64_slots(c, ev, _records(name)[0])
    want, bound = ev["value"][2:].astype(np.float64), ref.sum_bound(ev["n"], ev["abs"])[2:]
    assert (np.abs(got - want) <= bound).all(), (np.abs(got - want) / np.where(bound > 0, bound, 1)).max()
    assert (np.abs(ev["value"]) <= ev["abs"]).all()
    g, ph = ev["geometric"], ev["photometric"]
    assert np.abs((g[0] + ph[0] - ev["value"])[2:].astype(float)).max() <= 1e-17 * float(ev["abs"][2:].max())


@pytest.mark.parametrize("name", list(CASES))
def test_determinants_are_far_from_the_rule(name):
    """neither side's rounding can cross |det| < 1e-6: the reference's |det| lies outside [1e-9, 1e-3]"""
    ev, (U, info) = _eval(name)
    if ev["n"]:
        assert not (1e-9 <= abs(info["det"]) <= 1e-3), info["det"]
        assert info["solved"] == (abs(info["det"]) >= 1e-6)


def test_chunk_cases_have_the_sizes_that_take_each_branch():
    got = {c["name"]: (len(c["src"]) + cs.ICP_BLOCK - 1) // cs.ICP_BLOCK for c in cc.chunk_cases()}
    assert [got[f"ns{n}"] for n in (1, 63, 64, 65, 255, 256, 257)] == [1, 1, 1, 1, 1, 1, 2]
    assert [got[f"chunks{k}"] for k in (8, 16, 24, 9, 13)] == [8, 16, 24, 9, 13]
    for c in cc.chunk_cases():
        ev = _eval(c["name"])[0]
        assert len(c["tgt"]) == 500 and ev["n"] >= 0.9 * len(c["src"]) and len(c["sc"]) == len(c["src"])
        assert (_records(c["name"])[1] >= 4).all()                                # every target gradient is a solved one
    big = cc.large_case(256)
    assert len(big["src"]) == (3 * 256 + 1) * 256 + 17 and len(big["tgt"]) == 2000 and big["sc"].shape == big["src"].shape


def test_colours_are_tinted_fields_of_the_position():
    for c in cc.small_cases():
        if c["family"] == "singular" or c["name"].endswith("_hash"):
            continue
        assert np.array_equal(c["tc"], cc.tinted(cc.field(c["tgt"], c["centre"])))
        assert (c["tc"][:, 0] > c["tc"][:, 1]).all() and (c["tc"][:, 1] > c["tc"][:, 2]).all()
        assert c["tc"].min() > 0 and c["tc"].max() < 1 and c["sc"].min() > 0 and c["sc"].max() < 1
    c = CASES["lambda0.968"]                    # the source carries the colour of the place the true motion takes it to
    ev = _eval(c["name"])[0]
    assert np.abs(cr.intensity(c["sc"])[ev["i"]] - _records(c["name"])[0][ev["j"], 0]).max() < 0.02


def test_lambda_cases():
    assert [CASES[f"lambda{lam:g}"]["lam"] for lam in cc.LAMBDAS] == [0.0, 0.5, 0.968, 1.0]
    one, zero = _eval("lambda1")[0], _eval("lambda0")[0]
    c = CASES["lambda1"]
    plane = ref.evaluate(c["src"], c["tgt"], c["md"], ref.P2PLANE, None, None, c["tn"])
    assert np.array_equal(one["value"], plane["value"]) and np.array_equal(one["abs"], plane["abs"])
    assert not one["photometric"][0].any() and not one["photometric"][1].any()
    assert np.array_equal(zero["value"][2:], zero["photometric"][0][2:]) and not zero["geometric"][1][2:].any()
    assert zero["photometric"][0][2:].all()                                      # the photometric row reaches every slot
    assert one["n"] == zero["n"] == 600 == len(c["src"])


def test_permutation_cases_move_every_row_and_hashed_colours_show_a_wrong_gather():
    base = _eval("lambda0.968")[0]
    for name in ("reversed_smooth", "shuffled_smooth"):
        ev = _eval(name)[0]
        assert ev["n"] == base["n"]
        # the same pairs in another order: the sums agree to the summation's rounding
        assert (np.abs(ev["value"] - base["value"]).astype(float) <= ref.sum_bound(ev["n"], ev["abs"])).all()
    assert np.array_equal(CASES["reversed_smooth"]["src"], CASES["lambda0.968"]["src"][::-1])
    moved = CASES["shuffled_smooth"]["src"][:, None, :] == CASES["lambda0.968"]["src"][None, :, :]
    assert (moved.all(2).argmax(1) != np.arange(600)).mean() > 0.99
    for name in ("given_hash", "reversed_hash", "shuffled_hash"):
        c = CASES[name]
        k = c["sc"] * 1024
        assert np.array_equal(k, np.round(k)) and c["sc"].min() >= 0 and c["sc"].max() < 1
        assert np.abs(np.diff(cr.intensity(c["sc"]))).mean() > 0.1               # neighbouring rows are unrelated
        ev = _eval(name)[0]
        wrong = dict(src_intensity=np.roll(cr.intensity(c["sc"]), 1), tgt_records=_records(name)[0], lambda_geometric=c["lam"])
        ev_w = ref.evaluate(c["src"], c["tgt"], c["md"], ref.COLORED, c["init"], None, c["tn"], colors=wrong)
        ratio = np.abs(ev_w["value"] - ev["value"])[23:].astype(float) / ref.sum_bound(ev["n"], ev["abs"])[23:]
        assert ratio.max() > 1e9, ratio                                          # a gather off by one row: far beyond the bound


def test_mixed_case_has_both_kinds_of_pair():
    c = CASES["mixed_gradients"]
    rec, cnt = _records(c["name"])
    ev = _eval(c["name"])[0]
    assert (cnt[c["is_sparse"]] < 4).all() and not rec[c["is_sparse"], 1:].any()
    assert (cnt[~c["is_sparse"]] >= 4).mean() > 0.9
    zero = ~rec[ev["j"], 1:].any(1)
    assert ev["n"] == 600 and zero.sum() >= 250 and (~zero).sum() >= 250
    assert c["is_sparse"][ev["j"]].sum() == 300 and 20 <= c["is_sparse"].sum() < len(c["tgt"]) // 4


def test_masked_cases_mask_what_they_say():
    ev = _eval("half_far")[0]
    assert ev["n"] == 300 and (ev["i"] % 2 == 1).all()
    ev = _eval("chunk_of_zeros")[0]
    assert ev["n"] == 300 and (ev["i"] < 300).all() and len(CASES["chunk_of_zeros"]["src"]) == 900 == len(CASES["chunk_of_zeros"]["sc"])
    ev, (U, info) = _eval("no_correspondence")
    assert ev["n"] == 0 and np.array_equal(U, np.eye(4))


def test_init_case_starts_forty_degrees_away():
    c = CASES["init40"]
    assert np.degrees(np.arccos((np.trace(c["init"][:3, :3]) - 1) / 2)) == pytest.approx(40.0)
    ev, (U, info) = _eval("init40")
    assert ev["n"] == 300 and info["solved"] and np.abs(U[:3, :3] - cs.MOTION[:3, :3]).max() < 5e-3


def test_far_cases_compare_the_step_where_the_solve_keeps_six_digits():
    """cond(J^T J) grows with the square of the distance from the origin (the Jacobians are taken in world coordinates): the
    step is compared where 32 err_x < 1e-6"""
    conds = []
    for c, off in zip(cc.far_cases(), cs.OFFSETS):
        ev, (U, info) = _eval(c["name"])
        assert ev["n"] == 1000 and info["solved"]
        assert np.abs(c["tgt"].mean(0) - c["centre"]).max() < 0.05
        assert c["compare_step"] == (32 * info["err_x"] < 1e-6), (off, info["cond"], info["err_x"])
        conds.append(info["cond"])
        print(f"far offset {off:g}: cond {info['cond']:.3g}, step tolerance {ref.step_tolerance(info, ref.COLORED, U):.3g}")
    assert conds[0] < 1e3 and conds[1] > 1e5 and conds[2] > 1e9 and conds[3] > 1e13
    assert [c["compare_step"] for c in cc.far_cases()].count(True) >= 2


def test_scaled_normals_tell_the_projected_point_from_the_point():
    """the predicted intensity at p instead of p' = p - e n changes r_I by -sp e (d . n): nothing on the unit normals of the
    other cases, thousands of times the bound on this one"""
    def shift(name):
        c = CASES[name]
        ev, rec = _eval(name)[0], _records(name)[0]
        n, g = c["tn"][ev["j"]], rec[ev["j"], 1:]
        e, gn = ((ev["p"] - ev["t"]) * n).sum(1), (g * n).sum(1)
        m = -(g - gn[:, None] * n)
        J_i = np.sqrt(1.0 - c["lam"]) * np.concatenate([np.cross(ev["p"], m), m], 1)
        d_jtr = J_i.T @ (-np.sqrt(1.0 - c["lam"]) * e * gn)
        return float((np.abs(d_jtr) / ref.sum_bound(ev["n"], ev["abs"])[23:]).max())
    c = CASES["scaled_normals"]
    length = np.linalg.norm(c["tn"], axis=1)
    assert length.min() < 0.65 and length.max() > 1.35 and np.abs(length - 1).mean() > 0.1
    assert _eval("scaled_normals")[0]["n"] == 600 and _eval("scaled_normals")[1][1]["solved"]
    assert shift("scaled_normals") > 100 and shift("lambda0.968") < 0.01


def test_singular_case_is_exactly_singular():
    c = CASES["singular_plane"]
    ev, (U, info) = _eval(c["name"])
    rec = _records(c["name"])[0]
    assert ev["n"] == 300 and not rec[:, 1:].any() and (rec[:, 0] == 0.375).all()
    assert info["det"] == 0.0 and not info["solved"] and np.array_equal(U, np.eye(4))
    assert not ev["value"][[4, 5, 6]].any()                                       # the third to fifth columns of J are zero
