"""CPU tests of the TSDF restatement (tests/tsdf_ref.py): its two forms agree bit for bit, a plane comes back as a plane, and
pipeline.poses_from_edges composes a chain as test/check84.py does."""
import numpy as np
import pytest

from tests import rgbd_scene as sc
from tests import tsdf_ref as tr


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
