"""CPU tests of the TSDF restatement (tests/tsdf_ref.py): its two forms agree bit for bit, a plane comes back as a plane, and
pipeline.poses_from_edges composes a chain as test/check84.py does.  The test_edge_* tests run it at the inputs of
tests/test_tsdf_edges_gpu.py (tests/tsdf_cases.py) and pin the counts that show each case reaches its regime."""
import numpy as np
import pytest

from tests import rgbd_scene as sc
from tests import tsdf_cases as tc
from tests import tsdf_ref as tr
from tests.test_tsdf_gpu import POSES_A, _case_a
from tests.test_tsdf_gpu import _frame as _frame_a


def _frame(w, h, pose):
    inten, depth = sc.render(w, h, pose, sc.HOLES)
    return depth, np.repeat((inten * 255).astype(np.uint8)[..., None], 3, axis=2)


def test_literal_equals_vectorised():
    """A 24 x 18 frame twice (weights reach 2) from two poses into a coarse volume (a few dozen units: the literal form
    walks every voxel in Python): state after each frame and the extracted cloud are the same bits."""
    w, h = 24, 18
    cam = sc.camera(w, h)
    a, b = tr.Volume(0.03, 0.09, True, 4), tr.Volume(0.03, 0.09, True, 4)
    for pose in (np.eye(4), sc.TRUTH):
        depth, color = _frame(w, h, pose)
        a.integrate(depth, color, cam, np.linalg.inv(pose), literal=True)
        b.integrate(depth, color, cam, np.linalg.inv(pose), literal=False)
        sa, sb = a.state(), b.state()
        assert len(sa[0]) > 8 and sa[2].max() >= 1
        for x, y in zip(sa, sb):
            assert x.dtype == y.dtype and x.tobytes() == y.tobytes()
    assert a.state()[2].max() == 2
    ea, eb = a.extract_point_cloud(literal=True), b.extract_point_cloud(literal=False)
    assert len(ea[0]) > 100
    for x, y in zip(ea, eb):
        assert x.shape == y.shape and x.tobytes() == y.tobytes()


def test_plane_comes_back():
    """A fronto-parallel plane at 1 m: points within one voxel of z = 1, normals along +-z"""
    w, h, vl = 32, 24, 0.01
    cam = sc.camera(w, h)
    vol = tr.Volume(vl, 0.04, False, 4)
    vol.integrate(np.full((h, w), 1.0, np.float32), None, cam, np.eye(4))
    pts, nrm, col = vol.extract_point_cloud()
    assert col is None and len(pts) > 1000
    assert np.abs(pts[:, 2] - 1.0).max() < vl
    # inside the observed patch the gradient is the plane's; at its rim the weight-blind trilinear value
    # (QUIRK_TSDF_NORMAL_IGNORES_WEIGHT) mixes in zeros of never-observed voxels, so the rim is left out
    fx, fy, cx, cy = cam
    u, v = pts[:, 0] / pts[:, 2] * fx + cx, pts[:, 1] / pts[:, 2] * fy + cy
    inner = (u > 3) & (u < w - 4) & (v > 3) & (v < h - 4)
    assert inner.sum() > 500
    assert np.abs(np.abs(nrm[inner, 2]) - 1.0).max() < 0.02
    assert np.abs(np.linalg.norm(nrm, axis=1) - 1.0).max() < 1e-12


def test_negative_coordinates_floor():
    """unit indices are floors: a point just left of the origin belongs to unit -1"""
    vol = tr.Volume(0.01, 0.04, False, 1)
    depth = np.zeros((3, 3), np.float32)
    depth[1, 1] = 1.0
    E = np.eye(4)
    E[0, 3] = 0.05                # world x = camera x - 0.05: the sample sits at (-0.05, 0, 1), units are 0.16 m wide
    # x: [-0.09, -0.01] lies wholly in unit -1 (not 0: floor, not truncation); y: [-0.04, 0.04] straddles -1 and 0; z: [0.96, 1.04] in 6
    assert vol.touch(depth, (10.0, 10.0, 1.0, 1.0), E) == [(-1, -1, 6), (-1, 0, 6)]


# ---- the edge cases of tests/test_tsdf_edges_gpu.py: the restatement's two forms agree there too, and the counts that show each
# ---- case reaches its regime are pinned
def _same_bits(a, b, what):
    for x, y in zip(a, b):
        if x is None or y is None:
            assert x is None and y is None, what
        else:
            assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), what


def _both_forms(vl, trunc, stride, frames, cam):
    """frames: [(depth, colour, extrinsic)] into a literal and a vectorised volume -> the vectorised volume, both held equal"""
    a, b = tr.Volume(vl, trunc, True, stride), tr.Volume(vl, trunc, True, stride)
    for depth, color, E in frames:
        a.integrate(depth, color, cam, E, literal=True)
        b.integrate(depth, color, cam, E, literal=False)
        _same_bits(a.state(), b.state(), "state")
    _same_bits(a.extract_point_cloud(literal=True), b.extract_point_cloud(literal=False), "cloud")
    return b


def test_edge_counts_past_512_units():
    states, cloud = tc.case_j()
    assert tuple(len(s[0]) for s in states) == tc.COUNTS["j_units"] and len(cloud[0]) == tc.COUNTS["j_points"]
    assert len(states[0][0]) > 512                      # three tiles of k_tsdf_rank, three chunks of k_tsdf_unit_offsets


def test_edge_counts_far_from_the_origin():
    states, clouds = tc.case_l1()
    idx = states[0][0]
    assert len(idx) == tc.COUNTS["l1_units"] and len(clouds[0][0]) == tc.COUNTS["l1_points"]
    assert tuple(idx.min(0)) == tc.COUNTS["l1_lo"] and tuple(idx.max(0)) == tc.COUNTS["l1_hi"]
    both = states[1][0]
    assert len(both) == tc.COUNTS["l1_units"] + tc.COUNTS["m_units"]          # the far units and frame 0's near the origin
    assert np.abs(both).max(1).min() <= 10 and both[:, 0].min() == tc.COUNTS["l1_lo"][0]
    assert len(clouds[1][0]) > len(clouds[0][0])


def test_edge_index_limits():
    """each of the six frames lands in unit 2^20 - 1 or -2^20 on its axis; one unit length further out it is refused"""
    depth, color = tc.l2_frame()
    cam = sc.camera(tc.L2_W, tc.L2_H)
    all_six = tr.Volume(tc.VL, tc.TRUNC, True, 4)
    for n, (axis, index, t, beyond) in enumerate(tc.l2_translations()):
        vol = tr.Volume(tc.VL, tc.TRUNC, True, 4)
        vol.integrate(depth, color, cam, tc.extrinsic_at(t))
        idx, _, w, _ = vol.state()
        assert len(idx) == tc.COUNTS["l2_units"] and (idx[:, axis] == index).all()
        others = np.delete(idx, axis, 1)
        assert others.min() == -1 and others.max() == 0
        assert int((w != 0).sum()) == tc.COUNTS["l2_weighted"][axis]
        assert len(vol.extract_point_cloud()[0]) == tc.COUNTS["l2_points"]
        if n == 0:                                      # the literal form walks 4 units x 4096 voxels in Python
            _both_forms(tc.VL, tc.TRUNC, 4, [(depth, color, tc.extrinsic_at(t))], cam)
        with pytest.raises(OverflowError):
            tr.Volume(tc.VL, tc.TRUNC, True, 4).integrate(depth, color, cam, tc.extrinsic_at(beyond))
        all_six.integrate(depth, color, cam, tc.extrinsic_at(t))
    idx = all_six.state()[0]
    assert len(idx) == 24 and idx.min() == -tc.LIMIT and idx.max() == tc.LIMIT - 1
    assert len(all_six.extract_point_cloud()[0]) == 6 * tc.COUNTS["l2_points"]


def test_edge_refused_frame_would_add_units():
    """case M: the frame that is refused touches units the volume does not hold, so the abandoned pass claims table entries"""
    states, _ = _case_a()
    held = set(map(tuple, states[0][0].tolist()))
    assert len(held) == tc.COUNTS["m_units"]
    clean = tc.m_inf_depth()
    assert np.isinf(clean[tc.M_PIXEL]) and tc.M_PIXEL[0] % 4 == 0 and tc.M_PIXEL[1] % 4 == 0
    clean[tc.M_PIXEL] = 0
    touched = tr.Volume(tc.VL, tc.TRUNC, True, 4).touch(clean, sc.camera(64, 48), np.linalg.inv(POSES_A[2]))
    assert len(set(touched) - held) >= 8
    with pytest.raises(OverflowError):
        tr.Volume(tc.VL, tc.TRUNC, True, 4).touch(_frame_a(64, 48, 2)[0], sc.camera(64, 48), np.linalg.inv(tc.m_far_pose()))


def test_edge_nan_is_no_sample():
    nan, zero, valid = tc.n_depths()
    assert valid == tc.COUNTS["n_valid"] and np.isnan(nan[8, 12]) and np.isnan(nan).sum() == 13 * 18
    (s_nan, c_nan), (s_zero, c_zero) = tc.case_n()
    assert len(s_nan[0]) == tc.COUNTS["n_units"] and len(c_nan[0]) == tc.COUNTS["n_points"]
    _same_bits(s_nan, s_zero, "NaN against zero, state")
    _same_bits(c_nan, c_zero, "NaN against zero, cloud")
    # both forms on a 24 x 18 crop with a NaN patch that covers sampled and unsampled pixels, in a coarse volume
    color = np.ascontiguousarray(_frame_a(64, 48, 1)[1][6:24, 10:34])
    crop, crop0 = nan[6:24, 10:34].copy(), zero[6:24, 10:34].copy()
    assert np.isnan(crop[::4, ::4]).sum() >= 9 and (crop[::4, ::4] > 0).sum() >= 9
    cam = sc.camera(24, 18)
    a = _both_forms(0.03, 0.09, 4, [(crop, color, np.eye(4))], cam)
    b = _both_forms(0.03, 0.09, 4, [(crop0, color, np.eye(4))], cam)
    assert len(a.state()[0]) > 8
    _same_bits(a.state(), b.state(), "crop, NaN against zero")


@pytest.mark.parametrize("case", range(3))
def test_edge_tiny_images(case):
    w, h, stride, cam = tc.P_CASES[case]
    depth, color = tc.p_frame(w, h)
    vol = _both_forms(tc.VL, tc.TRUNC, stride, [(depth, color, np.eye(4))], cam)
    idx, _, wt, _ = vol.state()
    assert (len(idx), int((wt != 0).sum()), len(vol.extract_point_cloud()[0])) == tc.COUNTS["p"][case]


def test_poses_from_edges(r3d):
    """A hand-made chain of four cameras: the edges are made from known camera-to-world poses in both directions, and the
    poses come back; the forward direction is test/check84.py's own formula written out."""
    rng = np.random.default_rng(3)
    rel = [sc.pose(*rng.uniform(-3, 3, 3), rng.uniform(-0.05, 0.05, 3)) for _ in range(4)]
    truth = [np.eye(4)]
    for M in rel:
        truth.append(truth[-1] @ M)
    # as odometry_edges returns them: frame k+1 -> frame k, x_k = inv(pose_k) pose_k+1 x_k+1
    back = [dict(source=k + 1, target=k, T=np.linalg.inv(truth[k]) @ truth[k + 1], info=np.eye(6), uncertain=False) for k in range(4)]
    # as check84.py's loop has them: frame k -> frame k+1
    fwd = [dict(source=k, target=k + 1, T=np.linalg.inv(truth[k + 1]) @ truth[k]) for k in range(4)]
    odometry, script = np.eye(4), [np.eye(4)]
    for e in fwd:
        odometry = e["T"] @ odometry
        script.append(np.linalg.inv(odometry))
    for edges in (back, fwd):
        got = r3d.pipeline.poses_from_edges(edges)
        assert len(got) == 5 and np.array_equal(got[0], np.eye(4))
        for g, t, s, ref in zip(got, truth, script, tr.poses_from_edges(edges)):
            assert np.abs(g - t).max() < 1e-12 and np.abs(g - s).max() < 1e-12 and np.abs(g - ref).max() < 1e-12
    assert np.array_equal(r3d.pipeline.poses_from_edges(fwd)[3], script[3])
    assert len(r3d.pipeline.poses_from_edges([])) == 1
    with pytest.raises(ValueError):
        r3d.pipeline.poses_from_edges([dict(source=2, target=0, T=np.eye(4))])
