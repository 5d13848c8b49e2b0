"""GPU tests of the RGB-D odometry (csrc/odometry.hip) against the numpy restatement tests/rgbd_odometry_ref.py, stage by stage:
planes bit for bit, correspondence lists equal outside the fragile pixels the restatement reports, the 29 sums within the bound
of two float64 summation orders, full calls within 100 x the restatement's own sensitivity to its summation order.
Sizes: 67x45 (odd; levels 33x22, 16x11), 130x98 (rows of 65 and 32 pixels, straddling a wave), 160x120, one 640x480 case."""
import ctypes
import functools
import json
import os

import numpy as np
import pytest

from tests import rgbd_odometry_ref as ref
from tests import rgbd_scene as scene
from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu
SMALL = [(67, 45), (130, 98), (160, 120)]
EPS = 2.0 ** -53
# A 5 degree / 10 cm pose (3 degree pitch + 4 degree roll, t = (6, 8, 0) cm): at 1.5 m and a 60 degree lens the translation
# alone moves the image by 7 % of its width and 12 % of its height, so a band along two edges leaves it and about half of the
# pixels keep a correspondence.  The pose is chosen on the restatement alone: the step taken there agrees with itself under the
# two summation orders to 1.3e-13 or better on every size, level and term, an eighth of the 1e-12 asked of the device.  (A
# 5 degree yaw with 10 cm along x, both pushing the same way, keeps a fifth of the pixels; the colour-term step there is
# a rotation of tens of degrees that the restatement itself reproduces only to 1.8e-12.)
FAR = scene.pose(3.0, 0.0, 4.0, (0.06, 0.08, 0.0))
PERTURBED = scene.pose(0.3, -0.3, 0.25, (0.003, -0.003, 0.003))      # 0.5 degree / 5 mm from the identity


@functools.lru_cache(maxsize=None)
def _pair(w, h):
    return scene.pair(w, h)


@functools.lru_cache(maxsize=None)
def _prepared(w, h, levels=3):
    src, tgt, cam, _ = _pair(w, h)
    return ref.Prepared(src, tgt, cam, levels=levels)


def _same_bits(got, want, what):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    assert got.shape == want.shape, what
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), f"{what}: NaN positions differ at {int((gn != wn).sum())} pixels"
    bad = got.view(np.uint32)[~gn] != want.view(np.uint32)[~wn]
    assert not bad.any(), f"{what}: {int(bad.sum())} values differ in their bits"


def _check_prepare(r3d, src, tgt, cam, levels=3, **option):
    pr = ref.Prepared(src, tgt, cam, levels=levels, **option)
    its = (1,) * levels
    for gl in range(levels):
        got = r3d.cloud_ops.debug_rgbd_prepare(src, tgt, cam, grad_level=gl, iteration_number_per_pyramid_level=its, **option)
        if gl == 0:
            for l in range(levels):
                for k, name in enumerate(("intensity", "depth")):
                    _same_bits(got["source"][l][k], pr.src[l][k], f"source {name} level {l}")
                    _same_bits(got["target"][l][k], pr.tgt[l][k], f"target {name} level {l}")
            n = len(pr.corr_init)
            assert got["correspondences_init"] == n
            for g, w_ in zip(got["scales"], pr.scales):
                print(f"scale {g!r} vs {w_!r}: rel {abs(g - w_) / w_:.2e}, bound {4 * n * EPS:.2e}")
                assert abs(g - w_) <= 4 * n * EPS * abs(w_)
        for k, name in enumerate(("dI/dx", "dI/dy", "dD/dx", "dD/dy")):
            _same_bits(got["gradients"][k], pr.grads[gl][k], f"{name} level {gl}")


@pytest.mark.parametrize("w,h", SMALL + [(640, 480)])
def test_planes_bit_for_bit(r3d, w, h):
    src, tgt, cam, _ = _pair(w, h)
    _check_prepare(r3d, src, tgt, cam)


def test_four_levels_and_nan_input_planes(r3d):
    src, tgt, cam, _ = _pair(67, 45)
    d = src[1].copy()
    d[5:9, 40:50] = np.nan                       # NaN and 0 both mean "no measurement"
    _check_prepare(r3d, (src[0], d), tgt, cam, levels=4)


def test_raw_conversion_bit_for_bit(r3d):
    rng = np.random.default_rng(5)
    w, h = 67, 45
    color = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    depth = rng.integers(300, 2900, (h, w)).astype(np.uint16)
    # at, one below and one above depth_trunc (3.5 m) and depth_max (3.0 m below); 0 = no measurement
    depth[3, 3:10] = (3500, 3499, 3501, 3000, 2999, 3001, 0)
    depth[20:24, 30:36] = (3500, 3499, 3501, 3000, 2999, 3001)
    for col, bgr in ((color, False), (color, True), (color[..., 0].copy(), False)):
        img = r3d.cloud_ops.rgbd_image(col, depth, depth_scale=1000.0, depth_trunc=3.5, bgr=bgr)
        gi, gd = img.planes()
        wi, wd = ref.convert_raw(col, depth, 1000.0, 3.5, bgr)
        _same_bits(gi, wi, f"intensity bgr={bgr} channels={img.channels}")
        _same_bits(gd, wd, "depth")
        assert gd[3, 3] == np.float32(3.5) and gd[3, 4] > 0 and gd[3, 5] == 0 and gd[3, 9] == 0
    # the same boundary pixels through the preparation's depth_max = 3.0 rule
    cam = scene.camera(w, h)
    _check_prepare(r3d, (wi, wd), (wi, wd), cam, depth_max=3.0)
    clipped = ref.prepare(wi, wd, 0.0, 3.0, 1)[0][1]
    assert np.isnan(clipped[21:23, 32]).all() and np.isnan(clipped[21:23, 35]).all()     # 3501 mm and 3001 mm spread as NaN


def _as_map(corr, w, h):
    m = np.full((h, w), -1, np.int64)
    m[corr[:, 3], corr[:, 2]] = corr[:, 1].astype(np.int64) * w + corr[:, 0]
    return m


def _check_iteration(r3d, pr, src, tgt, cam, level, T, jacobian, option, strict=False):
    """one debug iteration against the restatement: list, count, sums, pose after the step"""
    got = r3d.cloud_ops.debug_rgbd_iteration(src, tgt, cam, level, T, jacobian=("hybrid", "color")[jacobian],
                                             iteration_number_per_pyramid_level=(1,) * pr.levels, **option)
    h, w = pr.src[level][1].shape
    corr, reach, n_fragile = pr.corr(level, T, want_fragile=True)
    assert n_fragile <= 1e-3 * w * h, f"{n_fragile} fragile source pixels of {w * h}"
    assert not (strict and n_fragile)
    # target row-major order, each target pixel once
    t_idx = got["corr"][:, 3].astype(np.int64) * w + got["corr"][:, 2]
    assert (np.diff(t_idx) > 0).all()
    gm, wm = _as_map(got["corr"], w, h), _as_map(corr, w, h)
    differ = (gm != wm) & ~reach
    assert not differ.any(), f"level {level}: {int(differ.sum())} target pixels hold another source pixel"
    if reach.any() and not np.array_equal(gm, wm):
        return got                                  # the lists differ at a fragile pixel: the sums are not comparable
    s, mag = pr.sums(level, T, corr, jacobian)
    n = len(corr)
    assert got["sums"][0] == n
    bound = 2 * (n + 16) * EPS * mag
    err = np.abs(got["sums"] - s)
    worst = np.max(err[1:] / np.maximum(bound[1:], 1e-300)) if n else 0.0
    print(f"{w}x{h} level {level} jacobian {jacobian}: n = {n}, worst |sum error| / bound = {worst:.3f}")
    assert (err[1:] <= bound[1:]).all()
    ok, U = (False, np.eye(4)) if n == 0 else ref.solve6_to_matrix(s)
    assert got["ok"] == ok
    want_T = U @ np.asarray(T, dtype=np.float64) if ok else np.eye(4)
    print(f"    pose after the step: max |dT| = {np.abs(got['T'] - want_T).max():.3e}")
    assert np.abs(got["T"] - want_T).max() <= 1e-12
    return got


@pytest.mark.parametrize("w,h", SMALL)
def test_correspondences_and_sums(r3d, w, h):
    src, tgt, cam, truth = _pair(w, h)
    pr = _prepared(w, h)
    for level in range(3):
        for T in (np.eye(4), truth, FAR):
            for jacobian in (ref.HYBRID, ref.COLOR):
                _check_iteration(r3d, pr, src, tgt, cam, level, T, jacobian, {})
    # the far pose really pushes a band out and keeps some pixels (a wide depth gate so that the list is not empty)
    prw = ref.Prepared(src, tgt, cam, depth_diff_max=0.5)
    got = _check_iteration(r3d, prw, src, tgt, cam, 0, FAR, ref.HYBRID, dict(depth_diff_max=0.5))
    assert 0 < len(got["corr"]) < 0.95 * (np.isfinite(prw.src[0][1]).sum())


@pytest.mark.parametrize("tz", [-0.2, 0.2])
def test_ties_go_to_the_smaller_source_index(r3d, tz):
    """A fronto-parallel plane of constant depth, R = I, t = (0, 0, tz): every z' is the same number.  tz = +0.2 shrinks the
    image towards the principal point, so many source pixels share a target pixel with exactly equal z'; tz = -0.2 spreads
    them.  No exclusions: the smaller source index wins everywhere."""
    w, h = 130, 98
    cam = scene.camera(w, h)
    inten = scene.render(w, h)[0]
    plane = np.full((h, w), 1.0, np.float32)
    T = np.eye(4)
    T[2, 3] = tz
    opt = dict(depth_diff_max=0.25)
    pr = ref.Prepared((inten, plane), (inten, plane), cam, **opt)
    for level in range(3):
        got = _check_iteration(r3d, pr, (inten, plane), (inten, plane), cam, level, T, ref.HYBRID, opt)
        want = pr.corr(level, T)
        assert np.array_equal(got["corr"], want)
        hl, wl = pr.src[level][1].shape
        if tz > 0:
            assert len(want) < 0.8 * wl * hl      # collisions happened
            # brute force: the winner of a target pixel is the smallest source index that lands there
            M, k = ref.projection(T, pr.cams[level])
            u, v = np.meshgrid(np.arange(wl, dtype=np.float64), np.arange(hl, dtype=np.float64))
            p = [1.0 * ((M[i * 3] * u + M[i * 3 + 1] * v) + M[i * 3 + 2]) + k[i] for i in range(3)]
            ut, vt = np.trunc(p[0] / p[2] + 0.5).astype(int), np.trunc(p[1] / p[2] + 0.5).astype(int)
            first = np.full(wl * hl, wl * hl, np.int64)
            np.minimum.at(first, (vt * wl + ut).reshape(-1), np.arange(wl * hl))
            gm = _as_map(got["corr"], wl, hl).reshape(-1)
            assert np.array_equal(gm[gm >= 0], first[first < wl * hl])


def test_nearer_surface_wins_at_a_depth_step(r3d):
    w, h = 130, 98
    cam = scene.camera(w, h)
    frame = scene.render(w, h, step=(0.5, 0.3))
    T = scene.pose(0.0, 0.0, 0.0, (0.06, 0.0, 0.0))      # the near half slides over the far half
    opt = dict(depth_diff_max=0.5)
    pr = ref.Prepared(frame, frame, cam, **opt)
    got = _check_iteration(r3d, pr, frame, frame, cam, 0, T, ref.HYBRID, opt)
    # brute force z-buffer over every candidate: the winner's z' is the smallest that reaches its target pixel
    d = pr.src[0][1].astype(np.float64)
    M, k = ref.projection(T, pr.cams[0])
    u, v = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    with np.errstate(invalid="ignore"):
        p = [d * ((M[i * 3] * u + M[i * 3 + 1] * v) + M[i * 3 + 2]) + k[i] for i in range(3)]
        fu, fv = p[0] / p[2] + 0.5, p[1] / p[2] + 0.5
        ok = ~np.isnan(d) & (fu > -1) & (fu < w) & (fv > -1) & (fv < h)
    ut, vt = np.trunc(fu[ok]).astype(int), np.trunc(fv[ok]).astype(int)
    dt = pr.tgt[0][1].astype(np.float64)[vt, ut]
    with np.errstate(invalid="ignore"):
        keep = np.abs(p[2][ok] - dt) <= 0.5
    zmin = np.full(w * h, np.inf)
    np.minimum.at(zmin, (vt * w + ut)[keep], p[2][ok][keep].astype(np.float32).astype(np.float64))
    cnt = np.bincount((vt * w + ut)[keep], minlength=w * h)
    c = got["corr"]
    zw = p[2][c[:, 1], c[:, 0]].astype(np.float32).astype(np.float64)
    assert np.array_equal(zw, zmin[c[:, 3].astype(np.int64) * w + c[:, 2]])
    contested = cnt[c[:, 3].astype(np.int64) * w + c[:, 2]] > 1
    near_won = (d[c[:, 1], c[:, 0]] < d.mean())[contested]
    assert contested.sum() > 20 and near_won.any()


LOOP_ITERS = {1: (10,), 3: (20, 10, 5), 4: (10, 10, 10, 5)}


@pytest.mark.parametrize("levels", [1, 3, 4])
@pytest.mark.parametrize("w,h", SMALL)
def test_full_calls(r3d, monkeypatch, w, h, levels):
    src, tgt, cam, truth = _pair(w, h)
    its = LOOP_ITERS[levels]
    first = True
    for init in (None, PERTURBED):
        for jacobian in (ref.HYBRID, ref.COLOR):
            opt = dict(levels=levels, iterations=its)
            monkeypatch.setattr(ref, "SUMS_REVERSED", False)
            want = ref.compute_rgbd_odometry(src, tgt, cam, init, jacobian, **opt)
            monkeypatch.setattr(ref, "SUMS_REVERSED", True)
            other = ref.compute_rgbd_odometry(src, tgt, cam, init, jacobian, **opt)
            monkeypatch.setattr(ref, "SUMS_REVERSED", False)
            got = r3d.cloud_ops.rgbd_odometry(src, tgt, cam, init, ("hybrid", "color")[jacobian], want_trace=True,
                                              iteration_number_per_pyramid_level=its)
            where = (want["failed_level"], want["failed_iteration"])
            assert want["success"] == other["success"] and where == (other["failed_level"], other["failed_iteration"])
            if not want["success"]:     # Open3D's |det| < 1e-6 rule on a small level (the colour term alone on 16 x 11 pixels)
                print(f"{w}x{h} levels {levels} jacobian {jacobian}: the restatement fails at level, iteration {where}")
                assert not got["success"] and (got["failed_level"], got["failed_iteration"]) == where
                assert np.array_equal(got["T"], np.eye(4)) and not got["trace"][len(want["trace"]):].any()
                assert np.abs(got["trace"][:len(want["trace"])] - np.array(want["trace"]).reshape(-1, 4, 4)).max(initial=0.0) < 1e-9
                continue
            sens = np.abs(want["T"] - other["T"]).max()
            tol = 100 * sens
            err = np.abs(got["T"] - want["T"]).max()
            print(f"{w}x{h} levels {levels} init {'identity' if init is None else 'perturbed'} jacobian {jacobian}: sensitivity {sens:.2e}, "
                  f"tolerance {tol:.2e}, |T - T_ref| {err:.2e}, pose error {ref.pose_error(got['T'], truth):.2e}")
            assert tol < 1e-3, "ill-conditioned case: replace it"
            assert got["success"] and (got["failed_level"], got["failed_iteration"]) == (-1, -1)
            assert err <= tol
            assert got["trace"].shape == (sum(its), 4, 4) and np.array_equal(got["trace"][-1], got["T"])
            assert got["correspondences_init"] == want["correspondences_init"]
            # the information matrix at the pose the device reached
            G, Gm, n = ref.information(_prepared(w, h, 1).src[0][1], _prepared(w, h, 1).tgt[0][1], got["T"], cam)
            if got["correspondences"] == n:
                assert (np.abs(got["info"] - G) <= 2 * (n + 16) * EPS * Gm).all()
            else:       # a fragile pixel at this pose: whole terms differ, a handful at the most
                assert abs(got["correspondences"] - n) <= 1e-3 * w * h
                assert np.abs(got["info"] - G).max() <= 1e-3 * np.abs(G).max()
            assert np.array_equal(got["info"], got["info"].T)
            if first:       # the same bits on every run
                again = r3d.cloud_ops.rgbd_odometry(src, tgt, cam, init, ("hybrid", "color")[jacobian], want_trace=True,
                                                    iteration_number_per_pyramid_level=its)
                for key in ("T", "info", "trace", "r2", "correspondences"):
                    assert np.array_equal(got[key], again[key]), key
                first = False


def _recorded():
    from PIL import Image
    color = np.asarray(Image.open(os.path.join(GOLDEN, "output84/color_00008.png")))
    depth = np.asarray(Image.open(os.path.join(GOLDEN, "output84/depth_00008.png"))).astype(np.uint16)
    k = json.load(open(os.path.join(GOLDEN, "camera_intrinsic.json")))
    return color, depth, k


def test_recorded_frame(r3d):
    """depth_00008.png + color_00008.png of tests/golden/output84, the only recorded colour frame, as source and target."""
    color, depth, k = _recorded()
    img = r3d.cloud_ops.rgbd_image(color, depth, depth_scale=1000.0, depth_trunc=3.0)
    ok, T, info = r3d.compute_rgbd_odometry(img, img, k)
    assert ok and np.array_equal(T, np.eye(4))
    assert np.array_equal(info, info.T) and info[3, 3] > 1e5
    # from a 0.5 degree / 5 mm init the restatement cuts the max-abs error against the identity 85.5-fold
    # (5.26e-3 -> 6.15e-5); the device must reach half of that factor
    ok, T, _ = r3d.compute_rgbd_odometry(img, img, k, PERTURBED)
    before, after = ref.pose_error(PERTURBED, np.eye(4)), ref.pose_error(T, np.eye(4))
    print(f"recorded frame: {before:.3e} -> {after:.3e} ({before / after:.1f}-fold)")
    assert ok and after * (85.5 / 2) <= before
    # the pose-graph helper: two equal frames give an identity edge that is certain
    cam = r3d.cloud_ops.depth_camera(k, depth_scale=1000.0)
    edge, = r3d.pipeline.odometry_edges([(color, depth), (color, depth)], cam)
    assert (edge["source"], edge["target"], edge["uncertain"]) == (1, 0, False) and np.array_equal(edge["T"], np.eye(4))


def test_failures_are_results_not_errors(r3d):
    src, tgt, cam, _ = _pair(67, 45)
    zero = np.zeros_like(src[1])
    far = (tgt[0], tgt[1] + np.float32(1.0))             # beyond depth_diff_max everywhere
    for s, t in (((src[0], zero), (tgt[0], zero)), (src, far)):
        res = r3d.cloud_ops.rgbd_odometry(s, t, cam, want_trace=True)
        want = ref.compute_rgbd_odometry(s, t, cam)
        assert not res["success"] and np.array_equal(res["T"], np.eye(4)) and np.array_equal(res["info"], np.eye(6))
        assert (res["failed_level"], res["failed_iteration"]) == (want["failed_level"], want["failed_iteration"]) == (0, -1)
        assert res["correspondences_init"] == 0 and not res["trace"].any()
    edge, = r3d.pipeline.odometry_edges([r3d.cloud_ops.rgbd_image(np.zeros((45, 67), np.uint8), np.zeros((45, 67), np.uint16))] * 2,
                                        r3d.cloud_ops.depth_camera(dict(fx=cam[0], fy=cam[1], ppx=cam[2], ppy=cam[3])))
    assert edge["uncertain"] and np.array_equal(edge["T"], np.eye(4))
    # a failure inside the loop: one row of depth leaves the coarsest level without a solvable system
    thin = zero.copy()
    thin[20:26] = tgt[1][20:26]
    res = r3d.cloud_ops.rgbd_odometry((tgt[0], thin), (tgt[0], thin), cam)
    want = ref.compute_rgbd_odometry((tgt[0], thin), (tgt[0], thin), cam)
    assert bool(res["success"]) == bool(want["success"])
    assert (res["failed_level"], res["failed_iteration"]) == (want["failed_level"], want["failed_iteration"])


def test_refusals(r3d):
    src, tgt, cam, _ = _pair(67, 45)
    co = r3d.cloud_ops
    with pytest.raises(r3d.R3DError) as e:
        co.rgbd_odometry(src, tgt, cam, levels=5, iteration_number_per_pyramid_level=(1, 1, 1, 1))
    assert e.value.code == -1
    tiny = (np.full((3, 3), 0.5, np.float32), np.full((3, 3), 1.0, np.float32))
    with pytest.raises(r3d.R3DError) as e:
        co.rgbd_odometry(tiny, tiny, cam)
    assert e.value.code == -1
    for bad in (dict(iteration_number_per_pyramid_level=(1, -1, 1)), dict(depth_diff_max=-1.0)):
        with pytest.raises(r3d.R3DError) as e:
            co.rgbd_odometry(src, tgt, cam, **bad)
        assert e.value.code == -1
    with pytest.raises(r3d.R3DError) as e:
        co.rgbd_odometry(src, tgt, (0.0, cam[1], cam[2], cam[3]))
    assert e.value.code == -1
    # a NULL plane and an unknown jacobian, straight at the C ABI
    ctx, prm = r3d.default_context(), co.odometry_params()
    T, st = np.empty((4, 4)), co.OdometryStats()
    p = [a.ctypes.data_as(ctypes.c_void_p) for a in (src[0], src[1], tgt[0], tgt[1])]
    lib = r3d._lib.load()
    call = lambda prm, planes: lib.r3d_rgbd_odometry_f32(ctx._h, ctypes.byref(prm), *planes, 67, 45, 67, *cam, None,
                                                         T.ctypes.data_as(ctypes.c_void_p), None, ctypes.byref(st), None)
    assert call(prm, p) == 0
    assert call(prm, [p[0], None, p[2], p[3]]) == -1
    prm.jacobian = 2
    assert call(prm, p) == -1
    assert lib.r3d_rgbd_odometry_f32(ctx._h, ctypes.byref(co.odometry_params()), *p, 67, 45, 66, *cam, None,
                                     T.ctypes.data_as(ctypes.c_void_p), None, ctypes.byref(st), None) == -1     # stride < w


def test_device_form_equals_host_form(r3d):
    src, tgt, cam, _ = _pair(130, 98)
    ctx = r3d.default_context()
    host = r3d.cloud_ops.rgbd_odometry(src, tgt, cam, want_trace=True)
    ptrs = [ctx.to_device(p) for p in (src[0], src[1], tgt[0], tgt[1])]
    try:
        dev = r3d.cloud_ops.rgbd_odometry_device((ptrs[0], ptrs[1]), (ptrs[2], ptrs[3]), 130, 98, cam, want_trace=True)
    finally:
        for p in ptrs:
            ctx.free(p)
    for key in ("success", "T", "info", "trace", "r2", "correspondences", "correspondences_init"):
        assert np.array_equal(host[key], dev[key]), key
