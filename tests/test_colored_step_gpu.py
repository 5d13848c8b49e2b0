"""The coloured registration step on the device (icp_setup's colour plumbing -> k_icp_eval<MODE_COLORED> -> k_icp_step ->
solve6_to_matrix) against mode 3 of tests/icp_step_ref.py, case by case (tests/colored_step_cases.py; tests/test_colored_step_ref.py
holds the cases' own conditions).

Every case makes the three assertions of tests/test_icp_step_gpu.py.
 1. r3d_debug_icp_sums_colored's 29 slots, entry by entry: the count equal, [1] and [2..28] within (n + 64) 2^-53 sum|terms| of the
    reference.  The reference takes the target records the device returned with the slots, so the bound is a pure summation
    bound; the records themselves must equal r3d_color_gradients' output bit for bit (tests/test_colored_icp_gpu.py judges that).
 2. registration_colored(max_iteration=1)["T"] against U_ref * init, every entry within step_tolerance (32 cond(J^T J) 2^-53 |x|,
    floor 1e-14 (1 + |t|)).  The far cases make this comparison where 32 err_x < 1e-6 (offsets 0 and 10) and print the tolerance
    otherwise: the Jacobians are taken in world coordinates and cond(J^T J) grows with the square of the offset.
 3. fitness, inlier_rmse and correspondences of that call against an evaluation at the returned pose.
Each test prints a line `ICPSTEP ...` with its error / bound (pytest -s)."""
import numpy as np
import pytest

from tests import colored_icp_ref as cr
from tests import colored_step_cases as cc
from tests import icp_step_ref as ref
from tests.test_icp_step_gpu import _large, _ratio

pytestmark = pytest.mark.gpu

CASES = {c["name"]: c for c in cc.small_cases()}
USED = list(range(1, 29))


def _call_kw(c):
    return dict(lambda_geometric=c["lam"], gradient_radius=c["radius"], gradient_max_nn=c["nn"])


def read_slots(r3d, c):
    """(slots, records, reference evaluation on those records) and the failures of the records' own checks"""
    ops = r3d.cloud_ops
    got, rec = ops.debug_icp_sums_colored(c["src"], c["sc"], c["tgt"], c["tn"], c["tc"], c["md"], c["init"], **_call_kw(c))
    radius, nn = cc.gradient_setup(c)
    inten, grad = ops.color_gradients(c["tgt"], c["tn"], c["tc"], radius, nn)
    fails = []
    if not (np.array_equal(rec[:, 0], inten) and np.array_equal(rec[:, 1:], grad)):
        fails.append("the records of the set-up differ from r3d_color_gradients'")
    if not np.array_equal(rec[:, 0], cr.intensity(c["tc"])):
        fails.append("target intensities differ from ((r + g) + b) / 3")
    return got, rec, fails


def check_case(r3d, c, pairs=None):
    ops = r3d.cloud_ops
    init = np.eye(4) if c["init"] is None else c["init"]
    # ---- 1: the slots
    got, rec, fails = read_slots(r3d, c)
    colors = dict(src_intensity=cr.intensity(c["sc"]), tgt_records=rec, lambda_geometric=c["lam"])
    ev = ref.evaluate(c["src"], c["tgt"], c["md"], ref.COLORED, init, None, c["tn"], pairs=pairs, colors=colors)
    n = ev["n"]
    want, bound = ev["value"].astype(np.float64), ref.sum_bound(n, ev["abs"])
    if got[0] != n:
        fails.append(f"count {got[0]} != {n}")
    err = np.abs(got - want)
    r_slots = _ratio(err[USED], bound[USED])
    worst = USED[int(np.argmax(np.where(bound[USED] > 0, err[USED] / np.where(bound[USED] > 0, bound[USED], 1), err[USED] > 0)))]
    if n == 0 and np.any(got != 0):
        fails.append(f"slots without a correspondence are not zero: {got}")
    if r_slots > 1:
        fails.append(f"slots: error / bound = {r_slots:.3g} at slot {worst}")
    # ---- 2: one step through the public call
    res = ops.registration_colored(c["src"], c["sc"], c["tgt"], c["tn"], c["tc"], c["md"], c["init"], max_iteration=1, **_call_kw(c))
    T = res["T"]
    U, info = ref.step(ev, ref.COLORED)
    Tw = U @ init
    tol = ref.step_tolerance(info, ref.COLORED, Tw)
    r_step = 0.0
    if n == 0 or not info["solved"]:
        if not np.array_equal(T, init):                               # the identity update leaves the pose as it was
            fails.append(f"pose moved by {np.abs(T - init).max():.3g} where the update is the identity")
    elif c["compare_step"]:
        r_step = np.abs(T - Tw).max() / tol
        if r_step > 1:
            fails.append(f"step: error / tolerance = {r_step:.3g} (tolerance {tol:.3g})")
    else:
        print(f"ICPSTEP case={c['name']}: step not compared, tolerance {tol:.3g} (cond {info['cond']:.3g}), difference {np.abs(T - Tw).max():.3g}")
    # ---- 3: the statistics, which are those of an evaluation at the returned pose
    ev2 = ref.evaluate(c["src"], c["tgt"], c["md"], ref.P2P, T)
    r_rmse = 0.0
    if res["correspondences"] != ev2["n"] or res["fitness"] != ev2["n"] / len(c["src"]):
        fails.append(f"correspondences {res['correspondences']} fitness {res['fitness']!r}: reference {ev2['n']} {ev2['n'] / len(c['src'])!r}")
    elif ev2["n"] == 0:
        if res["inlier_rmse"] != 0.0:
            fails.append(f"inlier_rmse {res['inlier_rmse']!r} without correspondences")
    else:
        r_rmse = _ratio(res["inlier_rmse"] - ref.rmse(ev2), ref.rmse_tolerance(ev2))
        if r_rmse > 1:
            fails.append(f"inlier_rmse {res['inlier_rmse']!r}: reference {ref.rmse(ev2)!r}, error / bound = {r_rmse:.3g}")
    print(f"ICPSTEP family={c['family']} case={c['name']} mode=3 lambda={c['lam']:g} n={n} slots={r_slots:.3g} (slot {worst}) step={r_step:.3g} "
          f"step_tol={tol:.3g} rmse={r_rmse:.3g}")
    return fails, got, rec, ev


@pytest.mark.parametrize("name", list(CASES))
def test_step_matches_the_reference(r3d, name):
    c = CASES[name]
    fails, got, rec, ev = check_case(r3d, c)
    ops = r3d.cloud_ops
    if c["family"] == "lambda" and c["lam"] == 1.0:
        # the header's promise: sg = 1 leaves every geometric product as point-to-plane forms it, the photometric row adds zeros
        plane, _ = ops.debug_icp_sums(c["src"], c["tgt"], c["md"], 1, c["init"], None, c["tn"])
        if not np.array_equal(got, plane):
            fails.append(f"lambda = 1 differs from point-to-plane's slots by {np.abs(got - plane).max():.3g}")
    if c["family"] == "lambda" and c["lam"] == 0.0:
        pv, pab = ev["photometric"]
        r = _ratio((got - pv.astype(np.float64))[2:], ref.sum_bound(ev["n"], pab)[2:])
        if r > 1:
            fails.append(f"lambda = 0: slots against the photometric row alone, error / bound = {r:.3g}")
    if c["family"] == "mixed":
        sparse = c["is_sparse"]
        if rec[sparse, 1:].any() or not rec[~sparse, 1:].any(1).mean() > 0.9:
            fails.append("mixed gradients: the sparse half's records are not exactly zero, or the dense half's are")
        # pairs on a zero record add geometric terms only (m = 0, so J_I = 0): the reference forms exactly that from the records
        zero = ~rec[ev["j"], 1:].any(1)
        if not (zero.sum() >= 250 and (~zero).sum() >= 250):
            fails.append(f"mixed gradients: {zero.sum()} pairs on zero records, {(~zero).sum()} on solved ones")
    if c["family"] == "singular":
        if rec[:, 1:].any() or got[[4, 5, 6]].any():
            fails.append("singular plane: gradients or the zero columns' slots are not exactly zero")
    assert not fails, "\n".join(fails)


def test_more_chunks_than_workgroups(r3d):
    """(3 CUs + 1) 256 + 17 sources: three workgroups per CU under the XCD split with more chunks than workgroups and a
    remainder, the source intensities gathered through a permutation of that length"""
    base, pairs = _large()
    fails, *_ = check_case(r3d, cc.colored(base), pairs)
    assert not fails, "\n".join(fails)


def test_read_out_refuses_like_the_registration(r3d):
    ops = r3d.cloud_ops
    c = CASES["ns63"]
    read = ops.debug_icp_sums_colored
    with pytest.raises(r3d.R3DError, match="debug_icp_sums_colored: source and target colours required"):
        read(c["src"], None, c["tgt"], c["tn"], c["tc"], 0.05)
    with pytest.raises(r3d.R3DError, match="debug_icp_sums_colored: target normals required"):
        read(c["src"], c["sc"], c["tgt"], None, c["tc"], 0.05)
    with pytest.raises(r3d.R3DError, match="lambda_geometric"):
        read(c["src"], c["sc"], c["tgt"], c["tn"], c["tc"], 0.05, lambda_geometric=-0.1)
    with pytest.raises(r3d.R3DError, match="gradient_max_nn"):
        read(c["src"], c["sc"], c["tgt"], c["tn"], c["tc"], 0.05, gradient_max_nn=129)
    with pytest.raises(r3d.R3DError, match="max_correspondence_distance"):
        read(c["src"], c["sc"], c["tgt"], c["tn"], c["tc"], 0.0)
    a, ra = read(c["src"], c["sc"], c["tgt"], c["tn"], c["tc"], 0.05)
    b, rb = read(c["src"], c["sc"], c["tgt"], c["tn"], c["tc"], 0.05, np.eye(4), gradient_radius=0.1, gradient_max_nn=30)
    assert np.array_equal(a, b) and np.array_equal(ra, rb)          # deterministic; no pose = identity; the documented defaults
