"""The numpy restatement of the RGB-D odometry contract (tests/rgbd_odometry_ref.py) on its own: it converges on the synthetic
height-field scene, keeps the identity, reports failure, and its named quirk changes what it is said to change.  No device."""
import numpy as np

from tests import rgbd_odometry_ref as ref
from tests import rgbd_scene as scene


def test_restatement_converges_on_the_height_field():
    src, tgt, cam, truth = scene.pair(160, 120)
    before = ref.pose_error(np.eye(4), truth)
    res = ref.compute_rgbd_odometry(src, tgt, cam)
    after = ref.pose_error(res["T"], truth)
    print(f"max-abs pose error {before:.3e} -> {after:.3e} ({before / after:.1f}-fold)")
    assert res["success"] == 1 and len(res["trace"]) == 35
    assert after * 5 <= before
    assert np.array_equal(res["trace"][-1], res["T"])


def test_render_with_its_default_camera_given_explicitly():
    """render and pair take a camera; camera(w, h) given explicitly is the frame every earlier test sees, bit for bit"""
    w, h = 67, 45
    for kw in (dict(), dict(cam_to_world=scene.TRUTH, holes=scene.HOLES), dict(step=(0.5, 0.3))):
        for a, b in zip(scene.render(w, h, **kw), scene.render(w, h, cam=scene.camera(w, h), **kw)):
            assert a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    src, tgt, cam, _ = scene.pair(w, h)
    src2, tgt2, cam2, _ = scene.pair(w, h, cam=scene.camera(w, h))
    assert cam == cam2 and all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(src + tgt, src2 + tgt2))
    fx, fy, cx, cy = scene.skewed_camera(w, h)
    assert fy == 0.85 * fx and (cx, cy) == (0.5 * w - 0.5 + 0.11 * w, 0.5 * h - 0.5 - 0.07 * h)
    assert not np.array_equal(scene.render(w, h, cam=(fx, fy, cx, cy))[1], scene.render(w, h)[1])


def test_restatement_converges_with_a_skewed_camera_and_tells_fx_from_fy():
    """fx != fy and an off-centre principal point: the restatement still converges, and given the camera with fx and fy
    swapped it answers 6e-3 away -- ten orders above the tolerance of a full call, so a swap inside a kernel cannot hide"""
    for w, h in ((67, 45), (160, 120)):
        cam = scene.skewed_camera(w, h)
        src, tgt, cam, truth = scene.pair(w, h, cam=cam)
        before = ref.pose_error(np.eye(4), truth)
        res = ref.compute_rgbd_odometry(src, tgt, cam)
        after = ref.pose_error(res["T"], truth)
        swapped = ref.compute_rgbd_odometry(src, tgt, (cam[1], cam[0], cam[2], cam[3]))
        moved = np.abs(res["T"] - swapped["T"]).max()
        print(f"{w}x{h}: max-abs pose error {before:.3e} -> {after:.3e} ({before / after:.1f}-fold); fx <-> fy moves T by {moved:.2e}")
        assert res["success"] == 1 and len(res["trace"]) == 35
        assert after * 4 <= before
        assert swapped["success"] == 1 and moved > 1e-3


def test_identical_frames_keep_the_identity_exactly():
    _, tgt, cam, _ = scene.pair(67, 45)
    res = ref.compute_rgbd_odometry(tgt, tgt, cam)
    assert res["success"] == 1
    assert np.array_equal(res["T"], np.eye(4))
    assert res["correspondences"] == res["correspondences_init"] > 0


def test_all_zero_depth_is_a_failure():
    src, tgt, cam, _ = scene.pair(67, 45)
    zero = np.zeros_like(src[1])
    res = ref.compute_rgbd_odometry((src[0], zero), (tgt[0], zero), cam)
    assert res["success"] == 0 and np.array_equal(res["T"], np.eye(4))
    assert (res["failed_level"], res["failed_iteration"]) == (0, -1)


def test_truncating_round_lands_in_column_zero(monkeypatch):
    """A plane pushed 0.8 columns to the left: source column 0 projects to -0.8 + 0.5 = -0.3, which the truncating
    conversion sends to column 0 (where it loses to nobody: column 1 lands at 0.7 -> 0 too and is farther by index only) and
    floor() sends out of the image."""
    w, h = 16, 8
    cam = (20.0, 20.0, 7.5, 3.5)
    d = np.full((h, w), 2.0, np.float32)
    T = np.eye(4)
    T[0, 3] = -0.8 * 2.0 / 20.0
    quirk = ref.correspondences(d, d, T, cam)
    monkeypatch.setattr(ref, "QUIRK_TRUNCATING_ROUND", False)
    plain = ref.correspondences(d, d, T, cam)
    # with the quirk columns 0 and 1 both land in target column 0 and the smaller source index wins; without it column 0 leaves
    assert len(quirk) == len(plain)
    q0, p0 = quirk[quirk[:, 2] == 0], plain[plain[:, 2] == 0]
    assert (q0[:, 0] == 0).all() and (p0[:, 0] == 1).all()
    assert not np.array_equal(quirk, plain)


def test_projection_of_the_identity_is_exact():
    M, k = ref.projection(np.eye(4), scene.camera(67, 45))
    assert tuple(M[6:]) == (0.0, 0.0, 1.0) and not k.any()
