"""GPU tests of the TSDF volume (csrc/tsdf.hip) against the numpy restatement tests/tsdf_ref.py.  After every integrate: the set
of unit indices equal, and the tsdf, weight and colour planes bit for bit (r3d_debug_tsdf_units).  After extraction: the count
equal, points and colours bit for bit (sums, products and quotients in a fixed order), normals within 2^-50 per component: their
six trilinear values are bit-equal inputs, the normalisation is one float64 square root and three divisions, each within 1 ulp,
and 2^-50 is 4 ulp of a unit-vector component.

Case A (64 x 48, three poses, voxel 0.01, truncation 0.04, stride 4, a pool that starts at 8 units and grows to 240) reaches
nearly every branch: unit indices from -6 to 10, voxels outside the image, on holes and behind the surface, weights up to 3,
neighbours in the next unit and in absent units.  The other cases add what A lacks."""
import ctypes
import functools

import numpy as np
import pytest

from tests import rgbd_scene as sc
from tests import tsdf_ref as tr

pytestmark = pytest.mark.gpu
VL, TRUNC = 0.01, 0.04
NORMAL_TOL = 2.0 ** -50
POSES_A = (np.eye(4), sc.TRUTH, sc.pose(-2, 3, 1, (0.05, 0.03, -0.04)))


@functools.lru_cache(maxsize=None)
def _frame(w, h, k):
    """-> depth float32 [h,w], colour uint8 [h,w,3] (the intensity plane x 255 in three channels) at POSES_A[k]"""
    inten, depth = sc.render(w, h, POSES_A[k], sc.HOLES)
    color = np.ascontiguousarray(np.repeat((inten * 255).astype(np.uint8)[..., None], 3, axis=2))
    return depth, color                       # (case C's channels differ, so a swapped or repeated channel shows there)


@functools.lru_cache(maxsize=None)
def _case_a():
    """the restatement's case A, computed once: states after each frame and the extracted cloud (read-only)"""
    vol = tr.Volume(VL, TRUNC, True, 4)
    cam = sc.camera(64, 48)
    states = []
    for k, pose in enumerate(POSES_A):
        depth, color = _frame(64, 48, k)
        vol.integrate(depth, color, cam, np.linalg.inv(pose))
        states.append(tuple(a.copy() for a in vol.state()))
    return states, vol.extract_point_cloud()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _check_state(volume, want, what):
    idx, t, w, c = volume.debug_units()
    widx, wt, ww, wc = want
    assert np.array_equal(idx, widx), f"{what}: unit sets differ ({len(idx)} vs {len(widx)})"
    assert len(volume) == len(widx)
    for name, g, r in (("tsdf", t, wt), ("weight", w, ww), ("colour", c, wc)):
        if r is None:
            assert g is None
            continue
        bad = _bits(g) != _bits(r)
        assert not bad.any(), f"{what}: {int(bad.sum())} {name} entries differ in their bits, first at {np.argwhere(bad)[0]}"


def _check_cloud(got, want, what):
    (p, n, c), (wp, wn, wc) = got, want
    assert len(p) == len(wp), f"{what}: {len(p)} points, {len(wp)} expected"
    assert np.array_equal(_bits(p), _bits(wp)), f"{what}: points differ"
    if wc is None:
        assert c is None
    else:
        assert np.array_equal(_bits(c), _bits(wc)), f"{what}: colours differ"
    d = float(np.abs(n - wn).max()) if len(p) else 0.0
    print(f"{what}: {len(p)} points, largest normal difference {d:.3e} (bound {NORMAL_TOL:.3e})")
    assert d <= NORMAL_TOL


def _run_case_a(r3d, volume):
    cam = sc.camera(64, 48)
    states, _ = _case_a()
    for k, pose in enumerate(POSES_A):
        depth, color = _frame(64, 48, k)
        volume.integrate_f32(depth, color, cam, np.linalg.inv(pose))
        _check_state(volume, states[k], f"case A frame {k}")


def _volume(r3d, color=True, stride=4, initial_units=8, vl=VL, trunc=TRUNC):
    kind = r3d.TSDFVolumeColorType.RGB8 if color else r3d.TSDFVolumeColorType.NoColor
    return r3d.ScalableTSDFVolume(vl, trunc, kind, depth_sampling_stride=stride, initial_units=initial_units)


def test_case_a(r3d):
    states, cloud = _case_a()
    assert [len(s[0]) for s in states] == [194, 202, 240] and states[2][0].min() == -6 and states[2][0].max() == 10
    assert states[2][2].max() == 3 and len(cloud[0]) == 37537
    with _volume(r3d) as volume:
        _run_case_a(r3d, volume)
        st = volume.stats()
        assert (st["units"], st["frames"], st["touched"]) == (240, 3, len(tr.Volume(VL, TRUNC).touch(_frame(64, 48, 2)[0], sc.camera(64, 48),
                                                                                                      np.linalg.inv(POSES_A[2]))))
        assert st["growths"] >= 3 and st["capacity"] >= 240          # 8 -> ... -> at least 240: several growths
        assert volume.point_count() == 37537
        _check_cloud(volume.extract_arrays(), cloud, "case A")
        pcd = volume.extract_point_cloud()
        assert isinstance(pcd, r3d.PointCloud) and pcd.has_normals() and pcd.has_colors() and len(pcd) == 37537


def test_case_b_behind_the_camera(r3d):
    """constant depth 0.03 m: the box reaches unit Z = -1, whose voxels all have camera z <= 0"""
    cam = sc.camera(32, 24)
    depth, color = np.full((24, 32), 0.03, np.float32), np.full((24, 32, 3), 77, np.uint8)
    ref = tr.Volume(VL, TRUNC, True, 4)
    ref.integrate(depth, color, cam, np.eye(4))
    idx, _, w, _ = ref.state()
    assert (idx[:, 2] == -1).any() and not w[idx[:, 2] == -1].any() and w.any()
    with _volume(r3d) as volume:
        volume.integrate_f32(depth, color, cam, np.eye(4))
        _check_state(volume, ref.state(), "case B")
        _check_cloud(volume.extract_arrays(), ref.extract_point_cloud(), "case B")


@pytest.mark.parametrize("stride", [1, 3, 4])
def test_case_c_sizes_off_the_stride(r3d, stride):
    w, h = 50, 37
    cam = sc.camera(w, h)
    inten, depth = sc.render(w, h, sc.TRUTH, sc.HOLES)
    color = np.ascontiguousarray(np.stack([(inten * 255).astype(np.uint8), (inten * 100).astype(np.uint8), (inten * 30).astype(np.uint8)], -1))
    ref = tr.Volume(VL, TRUNC, True, stride)
    ref.integrate(depth, color, cam, np.linalg.inv(sc.TRUTH))
    with _volume(r3d, stride=stride) as volume:
        volume.integrate_f32(depth, color, cam, np.linalg.inv(sc.TRUTH))
        _check_state(volume, ref.state(), f"case C stride {stride}")
        _check_cloud(volume.extract_arrays(), ref.extract_point_cloud(), f"case C stride {stride}")


def test_case_d_no_colour(r3d):
    cam = sc.camera(64, 48)
    ref = tr.Volume(VL, TRUNC, False, 4)
    with _volume(r3d, color=False) as volume:
        for k in (0, 1):
            depth, color = _frame(64, 48, k)
            ref.integrate(depth, None, cam, np.linalg.inv(POSES_A[k]))
            volume.integrate_f32(depth, None if k == 0 else color, cam, np.linalg.inv(POSES_A[k]))     # NULL is accepted, an image ignored
            _check_state(volume, ref.state(), f"case D frame {k}")
        got = volume.extract_arrays()
        assert got[2] is None
        _check_cloud(got, ref.extract_point_cloud(), "case D")
        pcd = volume.extract_point_cloud()
        assert pcd.has_normals() and not pcd.has_colors()


def test_case_e_empty_and_truncated(r3d):
    cam = sc.camera(64, 48)
    depth, color = _frame(64, 48, 0)
    with _volume(r3d) as volume:
        volume.integrate_f32(np.zeros((48, 64), np.float32), color, cam, np.eye(4))
        assert len(volume) == 0 and volume.stats()["frames"] == 1 and volume.stats()["touched"] == 0
        assert volume.point_count() == 0
        p, n, c = volume.extract_arrays()
        assert p.shape == n.shape == c.shape == (0, 3)
        assert len(volume.debug_units()[0]) == 0
    raw = np.round(depth * 1000.0).astype(np.uint16)
    cut = float(np.median(raw[raw > 0])) / 1000.0
    full, half = tr.depth_from_u16(raw, 1000.0, 10.0), tr.depth_from_u16(raw, 1000.0, cut)
    assert 0.3 < (half > 0).sum() / (full > 0).sum() < 0.7
    counts = []
    for trunc_m, plane in ((10.0, full), (cut, half)):
        ref = tr.Volume(VL, TRUNC, True, 4)
        ref.integrate(plane, color, cam, np.eye(4))
        with _volume(r3d) as volume:
            volume.integrate(r3d.cloud_ops.rgbd_image(color, raw, 1000.0, trunc_m), cam, np.eye(4))
            _check_state(volume, ref.state(), f"case E depth_trunc {trunc_m}")
            counts.append(len(volume))
    assert counts[1] < counts[0]


def test_case_f_twice_reset_and_two_volumes(r3d):
    cam = sc.camera(64, 48)
    depth, color = _frame(64, 48, 0)
    states, cloud = _case_a()
    with _volume(r3d) as volume, _volume(r3d, initial_units=16) as other:
        volume.integrate_f32(depth, color, cam, np.eye(4))
        _, t1, w1, c1 = volume.debug_units()
        volume.integrate_f32(depth, color, cam, np.eye(4))
        _, t2, w2, c2 = volume.debug_units()
        assert np.array_equal(w2, 2 * w1) and w1.max() == 1
        assert np.array_equal(_bits(t2), _bits(t1)) and np.array_equal(_bits(c2), _bits(c1))
        ref = tr.Volume(VL, TRUNC, True, 4)
        ref.integrate(depth, color, cam, np.eye(4))
        ref.integrate(depth, color, cam, np.eye(4))
        _check_state(volume, ref.state(), "the same frame twice")
        volume.reset()
        assert len(volume) == 0 and volume.point_count() == 0 and volume.stats()["frames"] == 0
        # case A in `volume`, case B's frame in `other`, turn by turn on one context
        b_depth, b_color = np.full((24, 32), 0.03, np.float32), np.full((24, 32, 3), 77, np.uint8)
        b_ref = tr.Volume(VL, TRUNC, True, 4)
        for k, pose in enumerate(POSES_A):
            d, c = _frame(64, 48, k)
            volume.integrate_f32(d, c, cam, np.linalg.inv(pose))
            other.integrate_f32(b_depth, b_color, sc.camera(32, 24), np.eye(4))
            b_ref.integrate(b_depth, b_color, sc.camera(32, 24), np.eye(4))
            _check_state(volume, states[k], f"case A after reset, frame {k}")
            _check_state(other, b_ref.state(), f"the other volume, frame {k}")
        _check_cloud(volume.extract_arrays(), cloud, "case A after reset")
        _check_cloud(other.extract_arrays(), b_ref.extract_point_cloud(), "the other volume")


def test_case_g_slot_order_does_not_show(r3d):
    """case A in two fresh volumes with different starting capacities (different growth histories, different slots): the same bytes"""
    outs = []
    for initial in (8, 300):
        with _volume(r3d, initial_units=initial) as volume:
            _run_case_a(r3d, volume)
            outs.append([a.tobytes() for a in volume.debug_units()] + [a.tobytes() for a in volume.extract_arrays()])
    assert outs[0] == outs[1]


def test_case_h_entry_points_agree(r3d):
    ctx = r3d.default_context()
    w, h = 64, 48
    cam = sc.camera(w, h)
    frames, planes = [], []
    for k in range(3):
        depth, color = _frame(w, h, k)
        raw = np.round(depth * 1000.0).astype(np.uint16)
        frames.append((color, raw))
        planes.append(tr.depth_from_u16(raw, 1000.0, 3.0))
    img = r3d.cloud_ops.rgbd_image(frames[0][0], frames[0][1], 1000.0, 3.0)
    assert np.array_equal(_bits(img.planes(ctx)[1]), _bits(planes[0])), "the raw depth conversion is not r3d_debug_rgbd_convert's"
    ref = tr.Volume(VL, TRUNC, True, 4)
    outs = []
    with _volume(r3d) as a, _volume(r3d) as b, _volume(r3d) as c:
        for k, pose in enumerate(POSES_A):
            E = np.linalg.inv(pose)
            ref.integrate(planes[k], frames[k][0], cam, E)
            a.integrate(r3d.cloud_ops.rgbd_image(frames[k][0], frames[k][1], 1000.0, 3.0), cam, E)
            b.integrate_f32(planes[k], frames[k][0], cam, E)
            d_depth, d_color = ctx.to_device(planes[k]), ctx.to_device(frames[k][0])
            try:
                c.integrate_device(d_depth, d_color, w, h, cam, E)
                ctx.sync()
            finally:
                ctx.free(d_depth)
                ctx.free(d_color)
            for name, v in (("uint16", a), ("float host", b), ("float device", c)):
                _check_state(v, ref.state(), f"{name} entry point, frame {k}")
        want = ref.extract_point_cloud()
        for v in (a, b, c):
            outs.append(v.extract_arrays())
            _check_cloud(outs[-1], want, "entry points")
        # the device form of the extraction
        n = len(want[0])
        d_out = [ctx.alloc(n * 24) for _ in range(3)]
        try:
            assert c.extract_device(d_out[0], d_out[1], d_out[2], n) == n
            for d, host in zip(d_out, (outs[0][0], outs[0][1], outs[0][2])):
                got = np.empty((n, 3))
                ctx.d2h(got, d)
                assert got.tobytes() == host.tobytes()
        finally:
            for d in d_out:
                ctx.free(d)
    camera = r3d.cloud_ops.depth_camera(dict(fx=cam[0], fy=cam[1], ppx=cam[2], ppy=cam[3]), depth_scale=1000.0, depth_trunc=3.0)
    fused = r3d.pipeline.tsdf_fuse(frames, camera, list(POSES_A), VL, TRUNC, color=True, initial_units=8)
    assert fused.points.tobytes() == outs[0][0].tobytes() and fused.normals.tobytes() == outs[0][1].tobytes()
    assert fused.colors.tobytes() == outs[0][2].tobytes()
    grey = r3d.pipeline.tsdf_fuse(frames, camera, list(POSES_A), VL, TRUNC, color=False)
    assert grey.points.tobytes() == outs[0][0].tobytes() and not grey.has_colors()


def test_case_i_refusals(r3d):
    ctx = r3d.default_context()
    lib = r3d._lib.load()
    T = r3d.TSDFVolumeColorType

    def code(fn, *args, **kw):
        with pytest.raises(r3d.R3DError) as e:
            fn(*args, **kw)
        assert str(e.value).split(":", 1)[1].strip(), "no message came through r3d_last_error"
        return e.value.code

    assert code(r3d.ScalableTSDFVolume, 0.0, TRUNC) == -1
    assert code(r3d.ScalableTSDFVolume, -0.01, TRUNC) == -1
    assert code(r3d.ScalableTSDFVolume, VL, 0.0) == -1
    assert code(r3d.ScalableTSDFVolume, VL, TRUNC, depth_sampling_stride=0) == -1
    assert code(r3d.ScalableTSDFVolume, VL, TRUNC, volume_unit_resolution=8) == -4
    assert code(r3d.ScalableTSDFVolume, VL, TRUNC, T.Gray32) == -4
    cam = sc.camera(64, 48)
    depth, color = _frame(64, 48, 0)
    h = ctypes.c_void_p()
    prm = r3d.tsdf.tsdf_params(VL, TRUNC)
    assert lib.r3d_tsdf_create(ctx._h, None, ctypes.byref(h)) == -1 and lib.r3d_tsdf_create(ctx._h, ctypes.byref(prm), None) == -1
    for name in ("r3d_tsdf_destroy", "r3d_tsdf_reset", "r3d_tsdf_integrate", "r3d_tsdf_integrate_f32", "r3d_tsdf_integrate_f32_dev", "r3d_tsdf_stats",
                 "r3d_tsdf_extract_point_cloud", "r3d_tsdf_extract_point_cloud_dev", "r3d_debug_tsdf_units"):
        fn = getattr(lib, name)
        args = [0 if t in (ctypes.c_int32, ctypes.c_int64) else 0.0 if t is ctypes.c_double else None for t in fn.argtypes[1:]]
        assert fn(ctx._h, *args) == -1, f"{name} took a NULL volume"
    with _volume(r3d) as volume:
        assert code(volume.integrate_f32, depth, None, cam, np.eye(4)) == -1                         # RGB8 without a colour image
        assert code(volume.integrate_f32, depth, color[..., :1], cam, np.eye(4)) == -1               # ... with one channel
        assert code(volume.integrate, r3d.cloud_ops.rgbd_image(color[..., 0], (depth * 1000).astype(np.uint16)), cam, np.eye(4)) == -1
        assert code(volume.integrate_f32, depth, color[:40], cam, np.eye(4)) == -1                   # images of different sizes
        assert code(volume.integrate_f32, depth, color[:, :60], cam, np.eye(4)) == -1
        assert code(volume.integrate_f32, depth, color, (0.0, 1.0, 0.0, 0.0), np.eye(4)) == -1
        assert code(volume.integrate_f32, depth, color, cam, np.zeros((4, 4))) == -1
        assert len(volume) == 0 and volume.stats()["frames"] == 0
        volume.integrate_f32(depth, color, cam, np.eye(4))
        before = [a.tobytes() for a in volume.debug_units()]
        n = volume.point_count()
        assert n > 1000
        xyz, nrm, col = (np.full((n - 1, 3), 7.0) for _ in range(3))
        got = ctypes.c_int64()
        args = [a.ctypes.data_as(ctypes.c_void_p) for a in (xyz, nrm, col)]
        assert code(ctx.call, "r3d_tsdf_extract_point_cloud", volume._h, n - 1, *args, ctypes.byref(got)) == -1
        assert got.value == n and all((a == 7.0).all() for a in (xyz, nrm, col)), "a refused extraction wrote"
        assert code(ctx.call, "r3d_tsdf_extract_point_cloud", volume._h, n, args[0], None, args[2], ctypes.byref(got)) == -1
        assert code(ctx.call, "r3d_debug_tsdf_units", volume._h, 1, None, None, None, None, ctypes.byref(got)) == -1
        assert [a.tobytes() for a in volume.debug_units()] == before
    with _volume(r3d, vl=1e-9, trunc=1e-9) as volume:          # 1.6e-8 m units: a sample at 1.5 m has index 9e7, outside +-2^20
        assert code(volume.integrate_f32, depth, color, cam, np.eye(4)) == -4
        assert len(volume) == 0 and volume.point_count() == 0
