"""GPU tests of the coloured registration (r3d_color_gradients, r3d_icp_colored, r3d_icp_colored_dev and the COLORED mode of the
multi-view fusion) against the numpy restatement in tests/colored_icp_ref.py.  Bars of the registration loop are those of
tests/test_cloud_gpu.py: iterations and correspondences equal, fitness 1e-12, inlier_rmse 1e-9, T 1e-8."""
import functools

import numpy as np
import pytest

from oracle import cloud_oracle as co
from tests import colored_icp_ref as cr

pytestmark = pytest.mark.gpu
TINT = (1.1, 1.0, 0.9)          # three distinct channels whose mean is the intensity field


@functools.lru_cache(maxsize=None)
def _scene(relief, tint=TINT):
    return cr.scene(relief=relief, tint=tint)


@functools.lru_cache(maxsize=None)
def _gradient_case(name):
    """(points, normals, colours, radius, max_nn) of one gradient case and its reference, computed once:
    float64 and long-double restatement on the SAME neighbour lists"""
    rng = np.random.default_rng(2)
    max_nn = 30
    if name in EDGE_CASES:
        pts, nrm, col, radius, max_nn = _edge_cloud(name)
    elif name == "table":        # 6000 points with radius 0.04: about 120 within the radius, so the max_nn = 30 cut is exercised
        _, _, pts, nrm, col, _ = _scene(1e-3)
        radius = 0.04
    else:                        # the sparse cloud (300 points uniform in a 2 m cube, radius 0.2) and its first 3 / 5 points
        n = {"sparse": 300, "n3": 3, "n5": 5}[name]
        pts = rng.uniform(0, 2, (300, 3))
        nrm = rng.standard_normal((300, 3))
        nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
        col = rng.uniform(0, 1, (300, 3))
        pts, nrm, col = pts[:n], nrm[:n], col[:n]
        radius = 0.2 if name == "sparse" else 3.0       # 3 m: the few points all see each other
    nb = co.hybrid_neighbors(pts, radius, max_nn)
    i64, g64, cnt = cr.color_gradients(pts, nrm, col, radius, max_nn, np.float64, nb)
    _, gld, _ = cr.color_gradients(pts, nrm, col, radius, max_nn, np.longdouble, nb)
    scale = np.maximum(1.0, np.linalg.norm(gld.astype(np.float64), axis=1))[:, None]
    gap = float((np.abs(g64 - gld).astype(np.float64) / scale).max())
    return pts, nrm, col, radius, i64, g64, cnt, scale, gap, max_nn


LINEAR_NN, QUADRATIC_NN = (4, 5, 8, 9, 30), (5, 8)
EDGE_CASES = (["line"] + [f"lattice_linear_nn{k}" for k in LINEAR_NN] + [f"lattice_quadratic_nn{k}" for k in QUADRATIC_NN]
              + ["duplicates", "n63", "n64", "n65", "n129", "table+10", "table+100", "table+1000"])
LINEAR_GRADIENT = (0.25, 0.5, 0.0)


def _lattice():
    gx, gy = np.meshgrid(np.arange(9) / 8.0, np.arange(9) / 8.0, indexing="ij")
    return np.column_stack([gx.ravel(), gy.ravel(), np.zeros(81)])


def _edge_cloud(name):
    """(points, normals, colours, radius, max_nn) of the cases at the gradient kernel's edges"""
    up = lambda n: np.tile([[0.0, 0.0, 1.0]], (n, 1))
    grey = lambda inten: np.repeat(inten[:, None], 3, 1)         # (I + I) + I = 3 I and 3 I / 3 = I exactly for these dyadic I
    if name == "line":           # rank 2 (the line's direction and the normal): the determinant is exactly zero
        pts = np.column_stack([np.arange(8) / 8.0, np.zeros(8), np.zeros(8)])
        return pts, up(8), np.random.default_rng(3).uniform(0, 1, (8, 3)), 1.0, 30
    if name.startswith("lattice"):
        pts = _lattice()         # spacing 1/8, radius 0.3: 4 neighbours at 1/8, 4 at sqrt(2)/8, 4 at 2/8, 8 at sqrt(5)/8: every cut is among ties
        x, y = pts[:, 0], pts[:, 1]
        inten = 0.25 * x + 0.5 * y + 0.125 if "linear" in name else x * x + 0.5 * x * y
        return pts, up(81), grey(inten), 0.3, int(name.split("nn")[1])
    if name == "duplicates":     # coincident pairs: a zero row of A, d2 = 0 ties between a point and its copy
        rng = np.random.default_rng(4)
        p, nrm = rng.uniform(0, 1, (150, 3)), rng.standard_normal((150, 3))
        nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
        return np.concatenate([p, p]), np.concatenate([nrm, nrm]), rng.uniform(0, 1, (300, 3)), 0.3, 30
    if name.startswith("table+"):
        _, _, pts, nrm, col, _ = _scene(1e-3)
        return pts + float(name[6:]) * np.array([1.0, -0.6, 0.8]), nrm, col, 0.04, 30
    n = int(name[1:])            # n63 .. n129: either side of KNN_BLOCK = 64 and of two blocks, every point sees every other: lists of
    rng = np.random.default_rng(n)                                 # min(n, 128), the longest the kernel keeps
    pts, nrm = rng.uniform(0, 1, (n, 3)), rng.standard_normal((n, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    return pts, nrm, rng.uniform(0, 1, (n, 3)), 3.0, 128


@pytest.mark.parametrize("name", ["table", "sparse", "n3", "n5"] + EDGE_CASES)
def test_gradients_match_the_restatement(r3d, name):
    """Tolerance: ten times the largest gap between the restatement evaluated in float64 and in long double (same neighbour
    lists), relative to max(1, |g|).  Measured on the CPU (x87 long double, 64-bit mantissa):
        table   gap 6.6e-13  bound 6.6e-12   (6000 points, every one solved on 30 neighbours, |g| up to 12)
        sparse  gap 5.3e-12  bound 5.3e-11   (27 of 300 solved on 4 to 6 neighbours, 273 zero)
        n3      gap 0        bound 0         (fewer than 4 neighbours everywhere: all zero)
        n5      gap 2.6e-16  bound 2.6e-15
    (the cofactor inverse loses cond(A^T A)^2: oblique normals and few neighbours are the loosest).  The kernel sums and solves
    in the restatement's order: on the MI355X its gradients equalled the float64 restatement's bit for bit in all four cases
    (error 0).  Zero gradients are exactly zero, on the same points.
    The cases at the kernel's edges (_edge_cloud), measured the same way:
        line                      gap 0        every determinant exactly zero (QUIRK_SINGULAR): all eight gradients zero
        lattice_linear_nn4..30    gap 5.6e-17 (nn5: 1.1e-16)  the restatement is within 1.2e-16 of (0.25, 0.5, 0) at every cut
        lattice_quadratic_nn5 / 8 gap 2.6e-16 / 2.1e-16   the list is cut among tied distances: the (d2, index) order decides
        duplicates                gap 3.0e-11  300 points, 150 coincident pairs, all solved on 6 to 30 neighbours
        n63 / n64 / n65 / n129    gap 4.5e-13 / 2.7e-13 / 4.0e-13 / 9.9e-13   max_nn = 128, lists of min(n, 128)
        table+10 / +100 / +1000   gap 8.2e-13 / 8.1e-13 / 7.8e-12   the table moved by c (1, -0.6, 0.8)
    Left out on purpose: zero normals on the duplicated cloud, where the restatement's own gap is above 1 and judges nothing."""
    pts, nrm, col, radius, i64, g64, cnt, scale, gap, max_nn = _gradient_case(name)
    inten, grad = r3d.cloud_ops.color_gradients(pts, nrm, col, radius, max_nn)
    err = float((np.abs(grad - g64) / scale).max())
    print(f"{name}: float64 / long double gap {gap:.3e}, bound {10 * gap:.3e}, kernel against the float64 restatement {err:.3e}, "
          f"{int((cnt >= 4).sum())} of {len(pts)} solved")
    np.testing.assert_array_equal(inten, i64)
    np.testing.assert_array_equal((grad == 0).all(1), (g64 == 0).all(1))
    assert ((grad == 0).all(1) | (cnt >= 4)).all()
    assert err <= 10 * gap
    if name == "sparse":
        assert 0 < (cnt >= 4).sum() < len(pts)
    if name.startswith("table"):
        assert (cnt == 30).all()
    if name == "line":
        assert (cnt == 8).all() and not g64.any() and not grad.any()
    if name.startswith("lattice"):
        assert (cnt == np.minimum(max_nn, _gradient_case("lattice_linear_nn30")[6])).all()      # 8 (corners) to 21 lie within the radius
        if "linear" in name:     # the case's own condition: any cut of the tied neighbours determines the plane's gradient
            assert np.abs(g64 - LINEAR_GRADIENT).max() <= 4 * 2.0 ** -53
    if name == "duplicates":
        assert np.array_equal(pts[:150], pts[150:]) and (cnt >= 4).sum() > 250
    if name in ("n63", "n64", "n65", "n129"):
        assert (cnt == min(len(pts), 128)).all()


def _same_loop(got, want):
    assert got["iterations"] == want["iterations"]
    assert got["correspondences"] == want["correspondences"]
    assert abs(got["fitness"] - want["fitness"]) < 1e-12 and abs(got["inlier_rmse"] - want["inlier_rmse"]) < 1e-9
    assert np.abs(got["T"] - want["T"]).max() < 1e-8


@pytest.mark.parametrize("relief", [0.0, 1e-3])
@pytest.mark.parametrize("lam", [0.968, 0.5])
def test_matches_the_restatement_iteration_for_iteration(r3d, relief, lam):
    s, sc, t, tn, tc, T = _scene(relief)
    # criteria 0: max_iteration is the count performed (the scene converges in three); 0: one evaluation, no update;
    # 7 / 8 / 9: either side of the batch of eight evaluations the host enqueues at a time
    for max_it in (0, 1, 3, 7, 8, 9, 12):
        kw = dict(lambda_geometric=lam, max_iteration=max_it, relative_fitness=0.0, relative_rmse=0.0)
        want = cr.registration_colored(s, sc, t, tn, tc, 0.02, **kw)
        got = r3d.cloud_ops.registration_colored(s, sc, t, tn, tc, 0.02, **kw)
        assert got["iterations"] == max_it and not got["converged"]
        _same_loop(got, want)
    want = cr.registration_colored(s, sc, t, tn, tc, 0.02, lambda_geometric=lam)
    got = r3d.cloud_ops.registration_colored(s, sc, t, tn, tc, 0.02, lambda_geometric=lam)
    _same_loop(got, want)
    assert got["converged"] and got["iterations"] <= 6
    e_t, e_r = cr.pose_error(got["T"], T)
    assert e_t < 1e-4 and e_r < 0.01


def test_colour_stops_the_slide_on_a_flat_textured_patch(r3d):
    s, sc, t, tn, tc, T = _scene(0.0)
    plane = r3d.cloud_ops.registration(s, t, 0.02, mode=r3d.cloud_ops.P2PLANE, max_iteration=50, target_normals=tn)
    col = r3d.cloud_ops.registration_colored(s, sc, t, tn, tc, 0.02, max_iteration=50)
    e_plane, e_col = cr.pose_error(plane["T"], T)[0], cr.pose_error(col["T"], T)[0]
    print(f"translation error: point-to-plane {e_plane * 1e3:.3f} mm after {plane['iterations']} iterations, "
          f"coloured {e_col * 1e3:.4f} mm after {col['iterations']}")
    assert e_col < 0.1 * e_plane


def test_lambda_one_is_point_to_plane(r3d):
    """the photometric row then adds exact zeros to every sum"""
    s, sc, t, tn, tc, _ = _scene(1e-3)
    for max_it in (1, 5, 30):
        want = r3d.cloud_ops.registration(s, t, 0.02, mode=r3d.cloud_ops.P2PLANE, max_iteration=max_it, target_normals=tn)
        got = r3d.cloud_ops.registration_colored(s, sc, t, tn, tc, 0.02, lambda_geometric=1.0, max_iteration=max_it)
        assert got["iterations"] == want["iterations"] and got["correspondences"] == want["correspondences"]
        assert np.abs(got["T"] - want["T"]).max() < 1e-12


def test_constant_colours_are_point_to_plane(r3d):
    """no texture: every gradient and every photometric residual is zero, the geometric rows are point-to-plane's times sqrt(lambda)"""
    s, _, t, tn, _, _ = _scene(1e-3)
    want = r3d.cloud_ops.registration(s, t, 0.02, mode=r3d.cloud_ops.P2PLANE, target_normals=tn)
    got = r3d.cloud_ops.registration_colored(s, np.full_like(s, 0.4), t, tn, np.full_like(t, 0.4), 0.02)
    assert np.abs(got["T"] - want["T"]).max() < 1e-9


@pytest.mark.parametrize("ns", [1, 63, 257])
def test_small_sources(r3d, ns):
    s, sc, t, tn, tc, _ = _scene(1e-3)
    want = cr.registration_colored(s[:ns], sc[:ns], t, tn, tc, 0.02)
    got = r3d.cloud_ops.registration_colored(s[:ns], sc[:ns], t, tn, tc, 0.02)
    _same_loop(got, want)
    assert got["correspondences"] > 0


def test_five_point_target(r3d):
    s, sc, t, tn, tc, _ = _scene(1e-3)
    near = np.argsort(np.linalg.norm(t[:, :2], axis=1))[:5]           # the five target points nearest the patch centre
    want = cr.registration_colored(s, sc, t[near], tn[near], tc[near], 0.02)
    got = r3d.cloud_ops.registration_colored(s, sc, t[near], tn[near], tc[near], 0.02)
    assert want["correspondences"] > 0
    _same_loop(got, want)


def test_no_overlap_and_initial_guess(r3d):
    s, sc, t, tn, tc, T = _scene(1e-3)
    far = r3d.cloud_ops.registration_colored(s, sc, t + np.array([0.0, 0.0, 10.0]), tn, tc, 0.02)
    assert far["fitness"] == 0.0 and far["correspondences"] == 0 and np.array_equal(far["T"], np.eye(4))
    init = cr.rigid_z(0.5, (0.005, -0.003, 0.0008))
    want = cr.registration_colored(s, sc, t, tn, tc, 0.02, init=init)
    got = r3d.cloud_ops.registration_colored(s, sc, t, tn, tc, 0.02, init=init)
    _same_loop(got, want)
    assert cr.pose_error(got["T"], T)[0] < 1e-4


def test_host_and_device_entry_points_agree(r3d):
    s, sc, t, tn, tc, _ = _scene(1e-3)
    ctx = r3d.default_context(0)
    host = r3d.cloud_ops.registration_colored(s, sc, t, tn, tc, 0.02, ctx=ctx)
    ptrs = [ctx.to_device(a) for a in (s, sc, t, tn, tc)]
    try:
        dev = r3d.cloud_ops.registration_colored_device(ptrs[0], ptrs[1], len(s), ptrs[2], ptrs[3], ptrs[4], len(t), 0.02, ctx=ctx)
    finally:
        ctx.sync()
        for p in ptrs:
            ctx.free(p)
    assert np.array_equal(dev["T"], host["T"])
    for k in ("iterations", "converged", "correspondences", "fitness", "inlier_rmse"):
        assert dev[k] == host[k]


def test_loud_refusals(r3d):
    s, sc, t, tn, tc, _ = _scene(1e-3)
    reg = r3d.cloud_ops.registration_colored
    with pytest.raises(r3d.R3DError, match="colours required"):
        reg(s, sc, t, tn, None, 0.02)
    with pytest.raises(r3d.R3DError, match="colours required"):
        reg(s, None, t, tn, tc, 0.02)
    with pytest.raises(r3d.R3DError, match="normals required"):
        reg(s, sc, t, None, tc, 0.02)
    with pytest.raises(r3d.R3DError, match="lambda_geometric"):
        reg(s, sc, t, tn, tc, 0.02, lambda_geometric=1.5)
    with pytest.raises(r3d.R3DError, match="gradient_max_nn"):
        reg(s, sc, t, tn, tc, 0.02, gradient_max_nn=129)
    with pytest.raises(r3d.R3DError, match="mode must be"):          # r3d_icp itself keeps refusing the new mode number
        r3d.cloud_ops.registration(s, t, 0.02, mode=r3d.cloud_ops.COLORED, target_normals=tn)
    with pytest.raises(r3d.R3DError, match="radius"):
        r3d.cloud_ops.color_gradients(t, tn, tc, 0.0, 30)


def test_fusion_registers_on_the_colours(r3d):
    import torch
    s, sc, t, tn, tc, _ = _scene(1e-3)
    other = cr.rigid_z(0.3, (0.002, -0.001, 0.0005))
    views = [(t[:3000], tn[:3000], tc[:3000]), (s[:2000], np.zeros((2000, 3)), sc[:2000]),
             (co.transform_points(other, s[2000:3500]), np.zeros((1500, 3)), sc[2000:3500])]
    local = {v: torch.from_numpy(np.stack(planes)).cuda() for v, planes in enumerate(views)}
    fused, Ts = r3d.pipeline.multi_view_fuse_tensors(local, 3, threshold=0.02, mode=r3d.cloud_ops.COLORED)
    torch.cuda.synchronize()
    assert fused.shape == (3, 6500, 3) and np.array_equal(Ts[0], np.eye(4))
    ctx = r3d.default_context(0)
    for v in (1, 2):
        a, ref = local[v], local[0]
        alone = r3d.cloud_ops.registration_colored_device(a[0].data_ptr(), a[2].data_ptr(), a.shape[1], ref[0].data_ptr(), ref[1].data_ptr(),
                                                          ref[2].data_ptr(), ref.shape[1], 0.02, ctx=ctx)
        assert np.array_equal(Ts[v], alone["T"]) and alone["fitness"] > 0.5
    assert np.abs(Ts[2] @ other - Ts[1]).max() < 1e-3             # both views land on view 0
    with pytest.raises(ValueError, match="COLORED"):
        r3d.pipeline.multi_view_fuse_tensors({v: local[v][:2].contiguous() for v in local}, 3, threshold=0.02, mode=r3d.cloud_ops.COLORED)
