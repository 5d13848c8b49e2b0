"""GPU tests of the RGB-D odometry (csrc/odometry.hip) at the edges its first suite leaves alone, against the numpy restatement
tests/rgbd_odometry_ref.py with that suite's helpers and tolerances: a camera with fx != fy and an off-centre principal point,
rows with padding straight at the C ABI (float, device and raw entries), pyramid levels that do not iterate, slab counts
around the eight-way split and the 256-slab staging round of k_odo_step, preparation at the 64 x 4 tile edge and on levels one
pixel wide or high, and the gates of the correspondence search.  Largest input: 322 x 206."""
import ctypes
import functools

import numpy as np
import pytest

from tests import rgbd_odometry_ref as ref
from tests import rgbd_scene as scene
from tests.test_rgbd_odometry_gpu import EPS, FAR, PERTURBED, SMALL, _check_iteration, _check_prepare, _same_bits

pytestmark = pytest.mark.gpu
JACOBIANS = ("hybrid", "color")
RESULT_KEYS = ("success", "failed_level", "failed_iteration", "T", "info", "trace", "r2", "correspondences", "correspondences_init")


@functools.lru_cache(maxsize=None)
def _skewed(w, h, holes=scene.HOLES):
    return scene.pair(w, h, holes=holes, cam=scene.skewed_camera(w, h))


@functools.lru_cache(maxsize=None)
def _skewed_prepared(w, h, levels=3):
    src, tgt, cam, _ = _skewed(w, h)
    return ref.Prepared(src, tgt, cam, levels=levels)


def _pivot_product(s):
    """the determinant as solve6_to_matrix takes it: the product of the LDLT pivots of JTJ"""
    A, q = np.zeros((6, 6)), 2
    for a in range(6):
        for c in range(a, 6):
            A[a, c] = A[c, a] = s[q]
            q += 1
    L, D, det = np.zeros((6, 6)), np.zeros(6), 1.0
    with np.errstate(all="ignore"):
        for j in range(6):
            D[j] = A[j, j] - sum(L[j, k] * L[j, k] * D[k] for k in range(j))
            det *= D[j]
            for i in range(j + 1, 6):
                v = A[i, j] - sum(L[i, k] * L[j, k] * D[k] for k in range(j))
                L[i, j] = v / D[j] if D[j] != 0 else 0.0
    return det


def _check_full_call(r3d, monkeypatch, src, tgt, cam, init, jacobian, its, what, rows=False, **option):
    """One call of the library against the restatement, as test_full_calls of the first suite compares them: T within 100 x the
    restatement's sensitivity to its summation order, or a failure at the same level and iteration; trace, counts and the
    information matrix at the pose the device reached; rows: every row of the trace too.  -> the device's result,
    |T - T_ref| / tolerance (None for a failure)"""
    opt = dict(option, levels=len(its), iterations=its)
    monkeypatch.setattr(ref, "SUMS_REVERSED", False)
    want = ref.compute_rgbd_odometry(src, tgt, cam, init, jacobian, **opt)
    monkeypatch.setattr(ref, "SUMS_REVERSED", True)
    other = ref.compute_rgbd_odometry(src, tgt, cam, init, jacobian, **opt)
    monkeypatch.setattr(ref, "SUMS_REVERSED", False)
    got = r3d.cloud_ops.rgbd_odometry(src, tgt, cam, init, JACOBIANS[jacobian], want_trace=True, iteration_number_per_pyramid_level=its, **option)
    where = (want["failed_level"], want["failed_iteration"])
    assert want["success"] == other["success"] and where == (other["failed_level"], other["failed_iteration"])
    assert got["trace"].shape == (sum(its), 4, 4)
    assert got["correspondences_init"] == want["correspondences_init"]
    if not want["success"]:
        print(f"{what}: the restatement fails at level, iteration {where}")
        assert not got["success"] and (got["failed_level"], got["failed_iteration"]) == where
        assert np.array_equal(got["T"], np.eye(4)) and np.array_equal(got["info"], np.eye(6))
        assert not got["trace"][len(want["trace"]):].any() and got["correspondences"] == 0
        assert np.abs(got["trace"][:len(want["trace"])] - np.array(want["trace"]).reshape(-1, 4, 4)).max(initial=0.0) < 1e-9
        return got, None
    sens = np.abs(want["T"] - other["T"]).max()
    tol = 100 * sens
    err = np.abs(got["T"] - want["T"]).max()
    ratio = err / tol if tol > 0 else 0.0
    print(f"{what}: sensitivity {sens:.2e}, tolerance {tol:.2e}, |T - T_ref| {err:.2e}, |T - T_ref| / tolerance = {ratio:.3f}")
    assert tol < 1e-3, "ill-conditioned case: replace it"
    assert got["success"] and (got["failed_level"], got["failed_iteration"]) == (-1, -1)
    assert err <= tol
    assert len(want["trace"]) == sum(its)
    if sum(its):
        assert np.array_equal(got["trace"][-1], got["T"])
    if rows and sum(its):
        # every pose on the way by the same rule, with the largest sensitivity of any row: an iteration that converges hides a
        # wrong first step from the final pose, not from its own row of the trace
        wt, ot = (np.array(r["trace"]).reshape(-1, 4, 4) for r in (want, other))
        row_tol = 100 * np.abs(wt - ot).max()
        row_err = np.abs(got["trace"] - wt).max()
        print(f"{what}: trace rows: tolerance {row_tol:.2e}, |trace - trace_ref| {row_err:.2e}, |trace - trace_ref| / tolerance = {row_err / max(row_tol, 1e-300):.3f}")
        assert row_err <= row_tol
    pr = ref.Prepared(src, tgt, cam, levels=1, **option)
    G, Gm, n = ref.information(pr.src[0][1], pr.tgt[0][1], got["T"], cam, pr.depth_diff_max)
    h, w = pr.src[0][1].shape
    if got["correspondences"] == n:
        assert (np.abs(got["info"] - G) <= 2 * (n + 16) * EPS * Gm).all()
    else:       # a fragile pixel at this pose: whole terms differ, a handful at the most
        assert abs(got["correspondences"] - n) <= 1e-3 * w * h
        assert np.abs(got["info"] - G).max() <= 1e-3 * np.abs(G).max()
    assert np.array_equal(got["info"], got["info"].T)
    return got, ratio


# ---- a camera with fx != fy and an off-centre principal point ---------------------------------------------------------------
@pytest.mark.parametrize("w,h", SMALL)
def test_skewed_camera_planes(r3d, w, h):
    """the camera enters no plane and no gradient: the same bits as the restatement, which never reads it there"""
    src, tgt, cam, _ = _skewed(w, h)
    _check_prepare(r3d, src, tgt, cam)


@pytest.mark.parametrize("w,h", SMALL)
def test_skewed_camera_iterations(r3d, w, h):
    """fx and fy enter apart in the projection, the source points and both Jacobian rows; the restatement reports no fragile
    pixel at these poses, so every list is compared whole and every set of sums is reached"""
    src, tgt, cam, truth = _skewed(w, h)
    pr = _skewed_prepared(w, h)
    for level in range(3):
        for T in (np.eye(4), truth, FAR):
            for jacobian in (ref.HYBRID, ref.COLOR):
                _check_iteration(r3d, pr, src, tgt, cam, level, T, jacobian, {}, strict=True)


@pytest.mark.parametrize("w,h", SMALL)
def test_skewed_camera_full_calls(r3d, monkeypatch, w, h):
    """Default iterations.  At 67 x 45 the colour term fails in the restatement on level 2 (iteration 4 from the identity,
    2 from the perturbed pose) under both summation orders: the device must fail there too."""
    src, tgt, cam, _ = _skewed(w, h)
    for init in (None, PERTURBED):
        for jacobian in (ref.HYBRID, ref.COLOR):
            _, ratio = _check_full_call(r3d, monkeypatch, src, tgt, cam, init, jacobian, (20, 10, 5),
                                        f"skewed {w}x{h} init {'identity' if init is None else 'perturbed'} jacobian {jacobian}")
            assert (ratio is None) == ((w, h) == (67, 45) and jacobian == ref.COLOR)


# ---- rows with padding, straight at the C ABI ---------------------------------------------------------------------------------
def _vp(a):
    if a is None or isinstance(a, int):
        return ctypes.c_void_p(a)
    return a.ctypes.data_as(ctypes.c_void_p)


def _padded(plane, stride, fill):
    """rows of `stride` elements; the padding holds a value that a read past the row's end would use, not one it would drop"""
    out = np.full((plane.shape[0], stride), fill, plane.dtype)
    out[:, :plane.shape[1]] = plane
    return out


def _stats_result(rc, T, info, trace, st):
    return rc, dict(success=bool(st.success), failed_level=st.failed_level, failed_iteration=st.failed_iteration, T=T, info=info, trace=trace,
                    r2=st.r2, correspondences=st.correspondences, correspondences_init=st.correspondences_init)


def _call_f32(r3d, entry, planes, w, h, stride, cam, its=(20, 10, 5), init=None):
    """r3d_rgbd_odometry_f32 on four host arrays, or r3d_rgbd_odometry_f32_dev on four device pointers -> rc, result"""
    co, ctx = r3d.cloud_ops, r3d.default_context()
    prm = co.odometry_params("hybrid", iteration_number_per_pyramid_level=its)
    T, info, trace, st = np.empty((4, 4)), np.empty((6, 6)), np.zeros((sum(its), 4, 4)), co.OdometryStats()
    rc = getattr(r3d._lib.load(), entry)(ctx._h, ctypes.byref(prm), *[_vp(p) for p in planes], w, h, stride, *cam, _vp(init), _vp(T), _vp(info),
                                         ctypes.byref(st), _vp(trace))
    return _stats_result(rc, T, info, trace, st)


def _call_raw(r3d, frames, w, h, depth_stride, color_stride, cn, bgr, cam, its=(20, 10, 5), init=None):
    """r3d_rgbd_odometry on (depth uint16, colour uint8) source and target arrays -> rc, result"""
    co, ctx = r3d.cloud_ops, r3d.default_context()
    prm = co.odometry_params("hybrid", iteration_number_per_pyramid_level=its)
    dc = co.DepthCamera(*cam, 1000.0, 3.0, 0, 0)
    T, info, trace, st = np.empty((4, 4)), np.empty((6, 6)), np.zeros((sum(its), 4, 4)), co.OdometryStats()
    (sd, sc), (td, tc) = frames
    rc = r3d._lib.load().r3d_rgbd_odometry(ctx._h, ctypes.byref(prm), _vp(sd), _vp(sc), _vp(td), _vp(tc), w, h, depth_stride, color_stride, cn,
                                           int(bgr), ctypes.byref(dc), _vp(init), _vp(T), _vp(info), ctypes.byref(st), _vp(trace))
    return _stats_result(rc, T, info, trace, st)


def _assert_same_result(a, b, what):
    for key in RESULT_KEYS:
        assert np.array_equal(a[key], b[key]), f"{what}: {key} differs"


@pytest.mark.parametrize("w,h", [(67, 45), (130, 98)])
def test_padded_rows_float_entries(r3d, w, h):
    """stride = w + 5 with depth 1.0 and intensity 0.9 in the padding: the host entry (hipMemcpy2D), the device entry (the stride
    of k_odo_gauss3) and the preparation give what the contiguous planes give"""
    src, tgt, cam, _ = _skewed(w, h)
    planes = [src[0], src[1], tgt[0], tgt[1]]
    stride = w + 5
    pads = [_padded(p, stride, np.float32(fill)) for p, fill in zip(planes, (0.9, 1.0, 0.9, 1.0))]
    rc, flat = _call_f32(r3d, "r3d_rgbd_odometry_f32", planes, w, h, w, cam)
    assert rc == 0 and flat["success"] and flat["trace"][-1].any()
    rc, host = _call_f32(r3d, "r3d_rgbd_odometry_f32", pads, w, h, stride, cam)
    assert rc == 0
    _assert_same_result(host, flat, "padded host planes")
    ctx = r3d.default_context()
    ptrs = [ctx.to_device(p) for p in pads]
    try:
        rc, dev = _call_f32(r3d, "r3d_rgbd_odometry_f32_dev", ptrs, w, h, stride, cam)
    finally:
        for p in ptrs:
            ctx.free(p)
    assert rc == 0
    _assert_same_result(dev, flat, "padded device planes")
    # r3d_debug_rgbd_prepare with the same padded rows: every pyramid plane and the level-0 gradients against the restatement
    pr = _skewed_prepared(w, h)
    shapes = [(h >> l, w >> l) for l in range(3)]
    offs = np.cumsum([0] + [a * b for a, b in shapes])
    pyr = [np.full(offs[-1], -7.0, np.float32) for _ in range(4)]
    grad, n, sc = np.empty(shapes[0] + (4,), np.float32), ctypes.c_int64(), np.zeros(2)
    prm = r3d.cloud_ops.odometry_params(iteration_number_per_pyramid_level=(1, 1, 1))
    rc = r3d._lib.load().r3d_debug_rgbd_prepare(ctx._h, ctypes.byref(prm), *[_vp(p) for p in pads], w, h, stride, *cam, None, *[_vp(p) for p in pyr],
                                                0, _vp(grad), ctypes.byref(n), _vp(sc))
    assert rc == 0 and n.value == len(pr.corr_init)
    for l in range(3):
        for k, name in enumerate(("source intensity", "source depth", "target intensity", "target depth")):
            want = (pr.src[l] if k < 2 else pr.tgt[l])[k & 1]
            _same_bits(pyr[k][offs[l]:offs[l + 1]].reshape(shapes[l]), want, f"padded {name} level {l}")
    for k in range(4):
        _same_bits(np.ascontiguousarray(grad[..., k]), pr.grads[0][k], f"padded gradient {k}")


@functools.lru_cache(maxsize=None)
def _raw_pair(w, h):
    """a skewed pair quantised to what a sensor gives: depth in millimetres, three colour channels that differ (red and blue
    apart, so that their order matters) and one grey channel"""
    src, tgt, cam, truth = _skewed(w, h)
    out = []
    for inten, depth in (src, tgt):
        i = inten.astype(np.float64)
        rgb = np.rint(255.0 * np.stack([i, 0.8 * i + 0.1, 1.0 - i], -1)).astype(np.uint8)
        out.append((np.rint(depth.astype(np.float64) * 1000.0).astype(np.uint16), rgb, np.rint(255.0 * i).astype(np.uint8)))
    return out[0], out[1], cam, truth


@pytest.mark.parametrize("w,h", [(67, 45), (130, 98)])
def test_raw_entry_against_the_float_entry_and_the_restatement(r3d, monkeypatch, w, h):
    """r3d_rgbd_odometry = k_odo_convert + the float entry's run: the same bits as r3d_rgbd_odometry_f32 on the converted planes,
    contiguous or padded (depth_stride = w + 3 elements, color_stride = w cn + 7 bytes), for RGB, BGR and one channel; and
    that float call meets the restatement on ref.convert_raw's planes, which ties the raw pose to the reference."""
    (sd, srgb, sgrey), (td, trgb, tgrey), cam, _ = _raw_pair(w, h)
    assert not np.array_equal(sd, td) and not np.array_equal(srgb, trgb)
    cases = [("rgb", srgb, trgb, 3, False), ("bgr", np.ascontiguousarray(srgb[..., ::-1]), np.ascontiguousarray(trgb[..., ::-1]), 3, True),
             ("grey", sgrey, tgrey, 1, False)]
    results = {}
    for name, sc, tc, cn, bgr in cases:
        simg, timg = (r3d.cloud_ops.rgbd_image(c, d, depth_scale=1000.0, depth_trunc=3.0, bgr=bgr) for c, d in ((sc, sd), (tc, td)))
        splanes, tplanes = simg.planes(), timg.planes()
        wsrc, wtgt = ref.convert_raw(sc, sd, 1000.0, 3.0, bgr), ref.convert_raw(tc, td, 1000.0, 3.0, bgr)
        for g, w_, what in zip(splanes + tplanes, wsrc + wtgt, ("source intensity", "source depth", "target intensity", "target depth")):
            _same_bits(g, w_, f"{name} {what}")
        if name == "bgr":       # the same planes as rgb (the bytes are swapped and so is the flag): the reference of rgb holds
            assert all(np.array_equal(a, b) for a, b in zip(splanes + tplanes, results["rgb_planes"]))
            flt = results["rgb"]
        else:
            flt, _ = _check_full_call(r3d, monkeypatch, wsrc, wtgt, cam, None, ref.HYBRID, (20, 10, 5), f"raw {name} {w}x{h}")
            assert flt["success"]
        results[name], results[name + "_planes"] = flt, splanes + tplanes
        rc, raw = _call_raw(r3d, ((sd, sc), (td, tc)), w, h, w, w * cn, cn, bgr, cam)
        assert rc == 0
        _assert_same_result(raw, flt, f"raw {name} against the float entry")
        ds, cs = w + 3, w * cn + 7
        pad_c = lambda c: _padded(c.reshape(h, w * cn), cs, np.uint8(230))       # 230 / 255 = 0.9
        rc, padded = _call_raw(r3d, ((_padded(sd, ds, np.uint16(1000)), pad_c(sc)), (_padded(td, ds, np.uint16(1000)), pad_c(tc))), w, h, ds, cs, cn,
                               bgr, cam)
        assert rc == 0
        _assert_same_result(padded, raw, f"padded raw {name}")
    assert not np.array_equal(results["grey"]["T"], results["rgb"]["T"])
    # refusals
    assert _call_raw(r3d, ((sd, srgb), (td, trgb)), w, h, w - 1, w * 3, 3, False, cam)[0] == -1
    assert _call_raw(r3d, ((sd, srgb), (td, trgb)), w, h, w, w * 3 - 1, 3, False, cam)[0] == -1
    assert _call_raw(r3d, ((sd, srgb), (td, trgb)), w, h, w, w * 3, 2, False, cam)[0] == -1


# ---- levels that do not iterate -------------------------------------------------------------------------------------------------
SKIPPED = [(0, 5, 0), (5, 0, 3), (0, 0, 4), (3, 0, 0), (0, 0, 0), (0, 0, 0, 3), (2, 0, 0, 2)]


@pytest.mark.parametrize("its", SKIPPED, ids=lambda its: "-".join(map(str, its)))
@pytest.mark.parametrize("camera", ["camera", "skewed_camera"])
def test_skipped_levels(r3d, monkeypatch, camera, its):
    """odo_run prepares M and k for the camera of the next launch: the first level that iterates, the next one that does, or
    level 0 for the information matrix.  A wrong choice projects with another level's camera."""
    src, tgt, cam, _ = scene.pair(67, 45, cam=getattr(scene, camera)(67, 45))
    for jacobian in (ref.HYBRID, ref.COLOR):
        got, ratio = _check_full_call(r3d, monkeypatch, src, tgt, cam, PERTURBED, jacobian, its, f"{camera} iterations {its} jacobian {jacobian}",
                                      rows=True)
        assert jacobian == ref.COLOR or ratio is not None       # the hybrid term succeeds in the restatement on all of these
        if not any(its):
            assert got["success"] and np.array_equal(got["T"], PERTURBED) and got["trace"].shape == (0, 4, 4)
            pr = ref.Prepared(src, tgt, cam, levels=1)
            G, Gm, n = ref.information(pr.src[0][1], pr.tgt[0][1], PERTURBED, cam)
            assert got["correspondences"] == n == (2747 if camera == "camera" else 2756)
            assert (np.abs(got["info"] - G) <= 2 * (n + 16) * EPS * Gm).all()


@pytest.mark.parametrize("camera", ["camera", "skewed_camera"])
def test_first_camera_when_the_coarsest_level_is_skipped(r3d, monkeypatch, camera):
    """Iterations (0, 5, 0) from the 5 degree / 10 cm pose.  From the perturbed init of the cases above the level-1 list is the
    same under the camera of level 1 and of level 2 (the pose moves no projection across a pixel edge), so a first launch
    prepared for the wrong level passes there; at this pose the two lists differ, which the restatement shows first."""
    src, tgt, cam, _ = scene.pair(67, 45, cam=getattr(scene, camera)(67, 45))
    pr = ref.Prepared(src, tgt, cam, FAR)
    right = pr.corr(1, FAR)
    wrong = ref.correspondences(pr.src[1][1], pr.tgt[1][1], FAR, pr.cams[2])
    assert len(right) > 300 and abs(len(right) - len(wrong)) > 50
    for jacobian in (ref.HYBRID, ref.COLOR):
        _, ratio = _check_full_call(r3d, monkeypatch, src, tgt, cam, FAR, jacobian, (0, 5, 0), f"{camera} iterations (0, 5, 0) from the far pose",
                                    rows=True)
        assert ratio is not None


# ---- slab counts of k_odo_step ----------------------------------------------------------------------------------------------------
def _reached_the_sums(got, pr, T):
    """_check_iteration returns before the sums when a fragile pixel makes the lists differ"""
    return np.array_equal(got["corr"], pr.corr(0, T))


@pytest.mark.parametrize("w,h,slabs", [(16, 16, 1), (17, 16, 2), (64, 28, 7), (64, 32, 8), (65, 32, 9)])
def test_slab_counts_around_the_eight_way_split(r3d, w, h, slabs):
    """One level.  Eight threads share a slot of k_odo_step: fewer slabs than parts, as many, one more.  On every size the
    restatement solves at both poses with both terms and reports no fragile pixel."""
    assert (w * h + 255) // 256 == slabs
    src, tgt, cam, truth = _skewed(w, h)
    pr = _skewed_prepared(w, h, 1)
    for T in (np.eye(4), truth):
        for jacobian in (ref.HYBRID, ref.COLOR):
            got = _check_iteration(r3d, pr, src, tgt, cam, 0, T, jacobian, {}, strict=True)
            assert got["ok"] and _reached_the_sums(got, pr, T)


@pytest.mark.parametrize("w,h,slabs", [(256, 256, 256), (257, 256, 257), (322, 206, 260)])
def test_slab_counts_around_a_staging_round(r3d, monkeypatch, w, h, slabs):
    """One level.  k_odo_step stages 256 slabs at a time: exactly one round, one slab more, and a partial second round, in the
    29-slot iterate forms and (by the full call) the 22-slot information form."""
    assert (w * h + 255) // 256 == slabs
    src, tgt, cam, truth = _skewed(w, h)
    pr = _skewed_prepared(w, h, 1)
    reached = 0
    for T in (np.eye(4), truth):
        for jacobian in (ref.HYBRID, ref.COLOR):
            got = _check_iteration(r3d, pr, src, tgt, cam, 0, T, jacobian, {})
            reached += _reached_the_sums(got, pr, T)
    assert reached >= 2, "no pose of this size reached the comparison of the sums"
    _, ratio = _check_full_call(r3d, monkeypatch, src, tgt, cam, None, ref.HYBRID, (2,), f"{w}x{h} one level, two iterations")
    assert ratio is not None


# ---- preparation at the tile and size edges ---------------------------------------------------------------------------------------
def _with_nan_at_the_borders(depth):
    """NaN touching each border; on an image too small to keep a measurement next to them (Gaussian3 spreads each NaN by one
    pixel) nothing is planted"""
    d = depth.copy()
    h, w = d.shape
    if w >= 8 and h >= 3:
        d[h // 2, 0] = np.nan                                # left
        d[(h - 1) // 2, w - 1] = np.nan                      # right
        d[0, w // 3:w // 3 + 1 + (w >= 16)] = np.nan         # top
        d[h - 1, 2 * w // 3:2 * w // 3 + 1 + (w >= 16)] = np.nan      # bottom
    return d


@pytest.mark.parametrize("w,h,levels", [(63, 3, 1), (64, 4, 2), (65, 5, 2), (128, 9, 3), (129, 8, 3), (1, 1, 1), (2, 2, 2), (8, 45, 4), (67, 8, 4)])
def test_prepare_at_tile_and_size_edges(r3d, w, h, levels):
    """widths and heights at the 64 x 4 tile of the preparation kernels, the smallest images the library accepts, and levels one
    pixel wide (8 x 45: level 3 is 1 x 5) or high (67 x 8: 8 x 1), where both clamped taps are the pixel itself"""
    src, tgt, cam, _ = _skewed(w, h, ())
    src, tgt = (src[0], _with_nan_at_the_borders(src[1])), (tgt[0], _with_nan_at_the_borders(tgt[1]))
    pr = ref.Prepared(src, tgt, cam, levels=levels)
    if w >= 8 and h >= 3:       # the NaN reached the coarsest level and left a measurement there
        assert np.isnan(pr.tgt[-1][1]).any() and not np.isnan(pr.tgt[-1][1]).all()
    _check_prepare(r3d, src, tgt, cam, levels=levels)


def test_prepare_depth_limits(r3d):
    """depth_min = 1.45 with depth_max = 1.55: values at, one float32 step below and one above each limit, and -1, -0 and +inf"""
    w, h = 67, 45
    lo, hi = np.float32(1.45), np.float32(1.55)
    below, above = (lambda v: np.nextafter(v, np.float32(0))), (lambda v: np.nextafter(v, np.float32(9)))
    plants = [lo, below(lo), above(lo), hi, below(hi), above(hi), np.float32(-1.0), np.float32(-0.0), np.float32(np.inf)]
    kept = [True, False, True, True, True, False, False, False, False]
    opt = dict(depth_min=1.45, depth_max=1.55)
    # on a plane of 1.5 the footprint of each planted pixel is its own: NaN exactly where the rule drops the value
    inten = scene.render(w, h)[0]
    flat = np.full((h, w), 1.5, np.float32)
    for k, v in enumerate(plants):
        flat[20, 4 + 6 * k] = v
    d0 = ref.prepare(inten, flat, 1.45, 1.55, 1)[0][1]
    assert [bool(~np.isnan(d0[20, 4 + 6 * k])) for k in range(len(plants))] == kept
    cam = scene.skewed_camera(w, h)
    _check_prepare(r3d, (inten, flat), (inten, flat), cam, **opt)
    # the height field, of which the limits keep a part
    src, tgt, cam, _ = _skewed(w, h)
    ds, dt = src[1].copy(), tgt[1].copy()
    for k, v in enumerate(plants):
        ds[10 + 3 * k, 30], dt[10 + 3 * k, 33] = v, v
    pr = ref.Prepared((src[0], ds), (tgt[0], dt), cam, **opt)
    finite = np.isfinite(pr.tgt[0][1]).mean()
    assert 0.1 < finite < 0.9 and len(pr.corr_init) > 100
    _check_prepare(r3d, (src[0], ds), (tgt[0], dt), cam, **opt)


@pytest.mark.parametrize("w,h,levels", [(8, 45, 4), (67, 8, 4), (4, 4, 3), (2, 2, 2), (1, 1, 1)])
def test_full_calls_on_tiny_levels_fail_where_the_restatement_fails(r3d, monkeypatch, w, h, levels):
    """The coarsest level holds a handful of pixels in one row or column: its 6 x 6 system is singular and the first solve fails.
    The case is kept only while the restatement's determinant is at least 100 x below Open3D's 1e-6, so that no rounding
    decides the branch."""
    src, tgt, cam, _ = _skewed(w, h, ())
    pr = ref.Prepared(src, tgt, cam, levels=levels)
    for jacobian in (ref.HYBRID, ref.COLOR):
        for rev in (False, True):
            monkeypatch.setattr(ref, "SUMS_REVERSED", rev)
            corr, s, _, ok, _ = pr.step(levels - 1, np.eye(4), jacobian)
            det = _pivot_product(s)
            print(f"{w}x{h} jacobian {jacobian} reversed {rev}: {len(corr)} correspondences on level {levels - 1}, determinant {det:.3e}")
            assert not ok and len(corr) > 0 and abs(det) <= 1e-8
        monkeypatch.setattr(ref, "SUMS_REVERSED", False)
        got, ratio = _check_full_call(r3d, monkeypatch, src, tgt, cam, None, jacobian, (2,) * levels, f"{w}x{h} jacobian {jacobian}")
        assert ratio is None and (got["failed_level"], got["failed_iteration"]) == (levels - 1, 0) and not got["trace"].any()
        assert got["correspondences_init"] > 0


# ---- the gates of the correspondence search -------------------------------------------------------------------------------------
def test_depth_diff_max_zero(r3d, monkeypatch):
    """Identical frames at the identity: z' = d exactly, so |z' - d_t| <= 0 keeps every pixel that has a depth.  1 mm along z
    keeps none."""
    _, tgt, cam, _ = _skewed(67, 45)
    opt = dict(depth_diff_max=0.0)
    pr = ref.Prepared(tgt, tgt, cam, **opt)
    for level in range(3):
        got = r3d.cloud_ops.debug_rgbd_iteration(tgt, tgt, cam, level, np.eye(4), iteration_number_per_pyramid_level=(1, 1, 1), **opt)
        want = pr.corr(level, np.eye(4))
        assert len(want) == np.isfinite(pr.src[level][1]).sum() > 0
        assert np.array_equal(got["corr"], want) and np.array_equal(want[:, :2], want[:, 2:])
        assert got["sums"][0] == len(want) and got["sums"][1] == 0.0       # equal frames: every residual is 0
    got, ratio = _check_full_call(r3d, monkeypatch, tgt, tgt, cam, None, ref.HYBRID, (20, 10, 5), "depth_diff_max 0, equal frames", **opt)
    assert ratio is not None and np.array_equal(got["T"], np.eye(4))
    assert got["correspondences"] == got["correspondences_init"] == np.isfinite(pr.src[0][1]).sum()
    shifted = scene.pose(t=(0.0, 0.0, 0.001))
    assert len(ref.Prepared(tgt, tgt, cam, init=shifted, **opt).corr_init) == 0
    got, ratio = _check_full_call(r3d, monkeypatch, tgt, tgt, cam, shifted, ref.HYBRID, (20, 10, 5), "depth_diff_max 0, 1 mm along z", **opt)
    assert ratio is None and (got["failed_level"], got["failed_iteration"]) == (0, -1)


@pytest.mark.parametrize("name,T", [("half turn about y", scene.pose(ry_deg=180.0)), ("two metres back", scene.pose(t=(0.0, 0.0, -2.0)))])
def test_points_behind_the_camera(r3d, monkeypatch, name, T):
    """z' <= 0 everywhere: an empty list, which is the failure (0, -1) and not an error"""
    src, tgt, cam, _ = _skewed(67, 45)
    pr = ref.Prepared(src, tgt, cam, init=T, depth_diff_max=10.0)
    assert len(pr.corr_init) == 0 and np.isfinite(pr.src[0][1]).sum() > 0
    for opt in ({}, dict(depth_diff_max=10.0)):       # the wide gate: nothing but z' > 0 drops these pixels
        got, ratio = _check_full_call(r3d, monkeypatch, src, tgt, cam, T, ref.HYBRID, (20, 10, 5), name, **opt)
        assert ratio is None and (got["failed_level"], got["failed_iteration"]) == (0, -1) and got["correspondences_init"] == 0


TRUNCATED = scene.pose(t=(-0.0207, -0.0246, 0.0))        # 0.8 pixels to the left and up at 1.5 m on 67 x 45 (fx 58.0, fy 49.3)


def test_truncating_round_on_the_device(r3d):
    """(int)(f + 0.5) truncates toward zero: a source pixel that projects to (-1.5, -0.5) lands in column or row 0 and may win
    it.  The restatement has at least 10 such winners at this pose and no fragile pixel; floor() would drop them all."""
    w, h = 67, 45
    src, tgt, cam, _ = _skewed(w, h)
    pr = _skewed_prepared(w, h)
    want = pr.corr(0, TRUNCATED)
    M, k = ref.projection(TRUNCATED, pr.cams[0])
    u, v = want[:, 0].astype(np.float64), want[:, 1].astype(np.float64)
    d = pr.src[0][1][want[:, 1], want[:, 0]].astype(np.float64)
    p = [d * ((M[i * 3] * u + M[i * 3 + 1] * v) + M[i * 3 + 2]) + k[i] for i in range(3)]
    fu, fv = p[0] / p[2] + 0.5, p[1] / p[2] + 0.5
    below = ((fu > -1) & (fu < 0)) | ((fv > -1) & (fv < 0))
    print(f"{int(below.sum())} of {len(want)} winners have a projection in (-1, 0)")
    assert below.sum() >= 10
    for jacobian in (ref.HYBRID, ref.COLOR):
        got = _check_iteration(r3d, pr, src, tgt, cam, 0, TRUNCATED, jacobian, {}, strict=True)
        assert np.array_equal(got["corr"], want)


def test_a_good_call_after_a_failed_one(r3d):
    """the failure flag lives in the state block of one call: the next call on the same context starts clean"""
    src, tgt, cam, _ = _skewed(67, 45)
    zero = np.zeros_like(src[1])
    before = r3d.cloud_ops.rgbd_odometry(src, tgt, cam, PERTURBED, want_trace=True)
    failed = r3d.cloud_ops.rgbd_odometry((src[0], zero), (tgt[0], zero), cam, PERTURBED, want_trace=True)
    after = r3d.cloud_ops.rgbd_odometry(src, tgt, cam, PERTURBED, want_trace=True)
    assert before["success"] and not failed["success"] and (failed["failed_level"], failed["failed_iteration"]) == (0, -1)
    _assert_same_result(after, before, "after a failed call")
