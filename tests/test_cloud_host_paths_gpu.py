"""The compaction cores behind the cloud entry points read their count back in two orders: count first, then arrays of exactly
that many rows (r3d_reproject_disparity, r3d_backproject_depth, r3d_model_append_depth), or everything enqueued over the upper
bound w * h and count and bounding box in one read-back (r3d_disparity_to_cloud_*, r3d_model_align_append_depth).  Both orders
run the same kernels on the same flags and scan, so they must give the same points, bit for bit and in the same order -- on
maps of one pixel, on a map that is no multiple of the 256-thread block, and with the only valid pixel first or last."""
import numpy as np
import pytest

from oracle import cloud_oracle as co

pytestmark = pytest.mark.gpu

W, H = 37, 23                        # 851 pixels: three full blocks of 256 and a part of a fourth
INVALID = -16                        # the matcher's marker (disparity -1 in x16 units)
# an ordinary rectified rig: focal length 40 px, principal point mid-image, 6 cm baseline; W = d / baseline > 0 for every valid d
Q = np.array([[1.0, 0, 0, -18.0], [0, 1.0, 0, -11.0], [0, 0, 0, 40.0], [0, 0, 1.0 / 0.06, 0]])
INTR = dict(fx=4.0, fy=4.5, ppx=2.0, ppy=1.0)


def _maps():
    rng = np.random.default_rng(7)
    full = rng.integers(16, 16 * 30, (H, W)).astype(np.int16)          # valid disparities: >= 16 in x16 units, no point at infinity
    half = np.where(rng.random((H, W)) < 0.5, full, INVALID).astype(np.int16)
    first, last = np.full((H, W), INVALID, np.int16), np.full((H, W), INVALID, np.int16)
    first[0, 0], last[-1, -1] = full[0, 0], full[-1, -1]
    return {"1x1_valid": np.array([[160]], np.int16), "1x1_invalid": np.array([[INVALID]], np.int16), "half_invalid": half,
            "first_pixel_only": first, "last_pixel_only": last}


MAPS = _maps()


@pytest.mark.parametrize("name", list(MAPS))
def test_reprojection_count_first_equals_upper_bound(r3d, name):
    disp = MAPS[name]
    h, w = disp.shape
    n_valid = int((disp >= 0).sum())
    assert n_valid == {"1x1_valid": 1, "1x1_invalid": 0, "first_pixel_only": 1, "last_pixel_only": 1}.get(name, n_valid)
    if name == "half_invalid":
        assert 300 < n_valid < 550
    ctx = r3d.default_context()
    count_first, pix = r3d.cloud_ops.reproject_disparity(disp, Q, 0, want_pixels=True, ctx=ctx)
    d_d = ctx.to_device(disp)
    try:
        upper, nrm = r3d.cloud_ops.disparity_to_cloud_device(d_d, w, h, Q, 0, None, None, 0, None, 0, ctx=ctx)
    finally:
        ctx.free(d_d)
    assert nrm is None
    assert count_first.shape == upper.shape == (n_valid, 3)
    np.testing.assert_array_equal(pix, np.flatnonzero(disp.ravel() >= 0))
    assert count_first.tobytes() == upper.tobytes()                     # bit for bit, same order
    assert np.isfinite(upper).all()


def test_registration_mode_refusals_keep_their_words(r3d):
    """Every entry point that takes a registration mode refuses a bad mode, a non-positive distance and missing normals before it
    touches the device, each under its own name and in these words."""
    co = r3d.cloud_ops
    ctx = r3d.default_context()
    p = np.random.default_rng(3).random((60, 3))
    nrm = np.tile([0.0, 0.0, 1.0], (60, 1))
    d_p, d_n = ctx.to_device(p), ctx.to_device(nrm)
    model, bare = co.ResidentModel(ctx), co.ResidentModel(ctx)
    cam = co.depth_camera(INTR)
    frame = _one_pixel_frame()
    MODE, DIST = "mode must be 0 (P2P), 1 (P2PLANE) or 2 (GICP)", "max_correspondence_distance must be > 0"
    NEEDS = "this mode needs normals (normal_max_nn > 0)"
    try:
        model.append(p, normals=nrm)
        bare.append(p)
        cases = [
            ("icp: " + MODE, lambda: co.registration(p, p, 0.02, mode=3, ctx=ctx)),
            ("icp: " + DIST, lambda: co.registration(p, p, 0.0, ctx=ctx)),
            ("icp: target normals required for this mode", lambda: co.registration(p, p, 0.02, mode=co.P2PLANE, ctx=ctx)),
            ("icp: source normals required for GICP", lambda: co.registration(p, p, 0.02, mode=co.GICP, target_normals=nrm, ctx=ctx)),
            ("icp_dev: " + MODE, lambda: co.registration_device(d_p, 60, d_p, 60, 0.02, mode=-1, ctx=ctx)),
            ("icp_dev: " + DIST, lambda: co.registration_device(d_p, 60, d_p, 60, -1.0, ctx=ctx)),
            ("icp_dev: target normals required for this mode", lambda: co.registration_device(d_p, 60, d_p, 60, 0.02, mode=co.GICP, d_source_normals=d_n, ctx=ctx)),
            ("icp_dev: source normals required for GICP", lambda: co.registration_device(d_p, 60, d_p, 60, 0.02, mode=co.GICP, d_target_normals=d_n, ctx=ctx)),
            ("debug_icp_sums: " + MODE, lambda: co.debug_icp_sums(p, p, 0.02, 3, ctx=ctx)),
            ("debug_icp_sums: " + DIST, lambda: co.debug_icp_sums(p, p, 0.0, co.P2P, ctx=ctx)),
            ("debug_icp_sums: target normals required for this mode", lambda: co.debug_icp_sums(p, p, 0.02, co.P2PLANE, ctx=ctx)),
            ("debug_icp_sums: source normals required for GICP", lambda: co.debug_icp_sums(p, p, 0.02, co.GICP, target_normals=nrm, ctx=ctx)),
            ("align: " + MODE, lambda: co.align_point_clouds(p, p, mode=3, ctx=ctx)),
            ("align: " + DIST, lambda: co.align_point_clouds(p, p, threshold=0.0, ctx=ctx)),
            ("align: " + NEEDS, lambda: co.align_point_clouds(p, p, mode=co.P2PLANE, normal_max_nn=0, ctx=ctx)),
            ("align: normal_max_nn > 128 not supported", lambda: co.align_point_clouds(p, p, mode=co.P2PLANE, normal_max_nn=129, ctx=ctx)),
            ("model_align_append: " + MODE, lambda: model.align_append(p, mode=3)),
            ("model_align_append: " + DIST, lambda: model.align_append(p, threshold=0.0)),
            ("model_align_append: " + NEEDS, lambda: model.align_append(p, mode=co.GICP, normal_max_nn=0)),
            ("model_align_append: normal_max_nn > 128 not supported", lambda: model.align_append(p, normal_max_nn=129)),
            ("model_align_append_depth: " + MODE, lambda: model.align_append_depth(frame, cam, mode=3)),
            ("model_align_append_depth: " + DIST, lambda: model.align_append_depth(frame, cam, threshold=0.0)),
            ("model_align_append_depth: " + NEEDS, lambda: model.align_append_depth(frame, cam, mode=co.P2PLANE, normal_max_nn=0)),
            ("model_register_append: " + MODE, lambda: model.register_append(p, mode=3)),
            ("model_register_append: " + DIST, lambda: model.register_append(p, threshold=0.0)),
            ("model_register_append: the model has no normals (r3d_model_estimate_normals)", lambda: bare.register_append(p, mode=co.P2PLANE)),
            ("model_register_append: source normals required for GICP", lambda: model.register_append(p, mode=co.GICP)),
        ]
        for words, call in cases:
            with pytest.raises(r3d.R3DError) as err:
                call()
            assert str(err.value).endswith(": " + words), (words, str(err.value))
        assert len(model) == len(bare) == 60                            # nothing was appended on the way
    finally:
        model.close()
        bare.close()
        ctx.free(d_p)
        ctx.free(d_n)


def _one_pixel_frame():
    d = np.zeros((3, 5), np.uint16)
    d[-1, -1] = 1234
    return d


def test_backprojection_of_a_last_pixel_direct_and_into_a_model(r3d):
    d = _one_pixel_frame()
    cam = r3d.cloud_ops.depth_camera(INTR)
    want, (v, u) = co.backproject(d, INTR)
    assert want.shape == (1, 3) and (v[0], u[0]) == (2, 4)
    pts, col, pix = r3d.cloud_ops.backproject_depth(d, cam, want_pixels=True)
    assert col is None and pix.tolist() == [14]
    model = r3d.cloud_ops.ResidentModel()
    try:
        assert model.append_depth(d, cam) == 1
        got, gc, gn = model.download()
    finally:
        model.close()
    assert gc is None and gn is None
    assert pts.shape == got.shape == (1, 3)
    assert pts.tobytes() == got.tobytes() == want.tobytes()


def test_an_empty_depth_frame_leaves_the_model_alone(r3d):
    cam = r3d.cloud_ops.depth_camera(INTR)
    model = r3d.cloud_ops.ResidentModel()
    try:
        assert model.append_depth(_one_pixel_frame(), cam) == 1
        before = model.download()[0]
        res = model.align_append_depth(np.zeros((3, 5), np.uint16), cam)
        after = model.download()[0]
    finally:
        model.close()
    np.testing.assert_array_equal(res["T"], np.eye(4))
    assert res["frame_points"] == 0 and res["appended"] == 0
    assert (res["fitness"], res["inlier_rmse"], res["iterations"], res["correspondences"], res["setup_ms"], res["loop_ms"]) == (0,) * 6
    assert res["converged"] is False
    assert before.tobytes() == after.tobytes()
