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
    if name == "table":          # 6000 points with radius 0.04: about 120 within the radius, so the max_nn = 30 cut is exercised
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
    nb = co.hybrid_neighbors(pts, radius, 30)
    i64, g64, cnt = cr.color_gradients(pts, nrm, col, radius, 30, np.float64, nb)
    _, gld, _ = cr.color_gradients(pts, nrm, col, radius, 30, np.longdouble, nb)
    scale = np.maximum(1.0, np.linalg.norm(gld.astype(np.float64), axis=1))[:, None]
    gap = float((np.abs(g64 - gld).astype(np.float64) / scale).max())
    return pts, nrm, col, radius, i64, g64, cnt, scale, gap


@pytest.mark.parametrize("name", ["table", "sparse", "n3", "n5"])
def test_gradients_match_the_restatement(r3d, name):
    """Tolerance: ten times the largest gap between the restatement evaluated in float64 and in long double (same neighbour
    lists), relative to max(1, |g|).  Measured on the CPU (x87 long double, 64-bit mantissa):
        table   gap 6.6e-13  bound 6.6e-12   (6000 points, every one solved on 30 neighbours, |g| up to 12)
        sparse  gap 5.3e-12  bound 5.3e-11   (27 of 300 solved on 4 to 6 neighbours, 273 zero)
        n3      gap 0        bound 0         (fewer than 4 neighbours everywhere: all zero)
        n5      gap 2.6e-16  bound 2.6e-15
    (the cofactor inverse loses cond(A^T A)^2: oblique normals and few neighbours are the loosest).  The kernel sums and solves
    in the restatement's order: on the MI355X its gradients equalled the float64 restatement's bit for bit in all four cases
    (error 0).  Zero gradients are exactly zero, on the same points."""
    pts, nrm, col, radius, i64, g64, cnt, scale, gap = _gradient_case(name)
    inten, grad = r3d.cloud_ops.color_gradients(pts, nrm, col, radius, 30)
    err = float((np.abs(grad - g64) / scale).max())
    print(f"{name}: float64 / long double gap {gap:.3e}, bound {10 * gap:.3e}, kernel against the float64 restatement {err:.3e}, "
          f"{int((cnt >= 4).sum())} of {len(pts)} solved")
    np.testing.assert_array_equal(inten, i64)
    np.testing.assert_array_equal((grad == 0).all(1), (g64 == 0).all(1))
    assert ((grad == 0).all(1) | (cnt >= 4)).all()
    assert err <= 10 * gap
    if name == "sparse":
        assert 0 < (cnt >= 4).sum() < len(pts)
    if name == "table":
        assert (cnt == 30).all()


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
