"""GPU tests of the TSDF volume (csrc/tsdf.hip) in the regimes tests/test_tsdf_gpu.py leaves out, against the same numpy
restatement (tests/tsdf_ref.py) with the same comparisons: unit sets equal, planes, points and colours bit for bit, normals
within NORMAL_TOL = 2^-50 (derived in that file's docstring).  The inputs and the restatement's counts are in tests/tsdf_cases.py;
tests/test_tsdf_ref.py holds the restatement's two forms equal at them and pins the counts on the CPU.

J  more than 256 and more than 512 units: the second and third tile of k_tsdf_rank, the carry of k_tsdf_unit_offsets, more than
   256 items in k_tsdf_assign and k_tsdf_rebuild, a growth that jumps to n_units + n_new, three growth histories with equal bytes
K  row strides larger than the row, through all three entry points, the padding filled with values that would show
L  unit indices of five digits, and of exactly 2^20 - 1 and -2^20 on every axis; one unit further out is refused
M  a frame refused on a volume that holds units, after its touch pass claimed table entries (and, in M3, overflowed the table)
N  NaN depth is no sample
P  images smaller than the sampling stride, a 1 x 1 image, a principal point at 0"""
import ctypes

import numpy as np
import pytest

from tests import rgbd_scene as sc
from tests import tsdf_cases as tc
from tests import tsdf_ref as tr
from tests.test_tsdf_gpu import POSES_A, TRUNC, VL, _case_a, _check_cloud, _check_state, _frame, _run_case_a, _volume

pytestmark = pytest.mark.gpu
_vp = ctypes.c_void_p


def _refused(r3d, fn, *args):
    """-> the code of the R3DError that fn raises; its message must be non-empty"""
    with pytest.raises(r3d.R3DError) as e:
        fn(*args)
    assert str(e.value).split(":", 1)[1].strip(), "no message came through r3d_last_error"
    return e.value.code


def _snapshot(volume, cloud=True):
    st = volume.stats()
    out = [len(volume), st["frames"], st["units"]] + [None if a is None else a.tobytes() for a in volume.debug_units()]
    if cloud:
        out += [volume.point_count()] + [None if a is None else a.tobytes() for a in volume.extract_arrays()]
    return out


# ---- J -----------------------------------------------------------------------------------------------------------------------------
def test_case_j_past_512_units(r3d):
    ctx = r3d.default_context()
    states, cloud = tc.case_j()
    assert tuple(len(s[0]) for s in states) == tc.COUNTS["j_units"] and len(cloud[0]) == tc.COUNTS["j_points"]
    cam = sc.camera(64, 48)
    n = len(cloud[0])
    outs = []
    for initial in (1, 8, 600):
        with _volume(r3d, initial_units=initial, vl=tc.J_VL, trunc=tc.J_TRUNC) as volume:
            for k in (0, 1):
                depth, color = _frame(64, 48, k)
                volume.integrate_f32(depth, color, cam, np.linalg.inv(POSES_A[k]))
                _check_state(volume, states[k], f"case J from {initial} units, frame {k}")
            st = volume.stats()
            assert st["units"] == 576 and st["capacity"] >= st["units"]
            assert (st["growths"] == 0) if initial == 600 else (st["growths"] >= 1)
            assert volume.point_count() == n
            got = volume.extract_arrays()
            _check_cloud(got, cloud, f"case J from {initial} units")
            d_out = [ctx.alloc(n * 24) for _ in range(3)]
            try:
                assert volume.extract_device(d_out[0], d_out[1], d_out[2], n) == n
                for d, host in zip(d_out, got):
                    back = np.empty((n, 3))
                    ctx.d2h(back, d)
                    assert back.tobytes() == host.tobytes()
            finally:
                for d in d_out:
                    ctx.free(d)
            outs.append([a.tobytes() for a in volume.debug_units()] + [a.tobytes() for a in got])
            volume.reset()
            assert len(volume) == 0 and volume.point_count() == 0 and volume.stats()["frames"] == 0
            depth, color = _frame(64, 48, 0)
            volume.integrate_f32(depth, color, cam, np.linalg.inv(POSES_A[0]))
            _check_state(volume, states[0], f"case J from {initial} units, frame 0 after reset")
    assert outs[0] == outs[1] == outs[2]


# ---- K -----------------------------------------------------------------------------------------------------------------------------
def test_case_k_padded_rows(r3d):
    ctx = r3d.default_context()
    w, h = tc.K_W, tc.K_H
    cam = sc.camera(w, h)
    E = np.ascontiguousarray(np.linalg.inv(sc.TRUTH))
    depth, color = tc.case_k_images()
    ds, cs = w + tc.K_DPAD, 3 * w + tc.K_CPAD
    pdepth = tc.padded(depth, ds, np.float32(9.0))                   # a positive depth in the padding would create units
    pcolor = tc.padded(color.reshape(h, 3 * w), cs, np.uint8(255))
    raw = np.round(depth * 1000.0).astype(np.uint16)
    praw = tc.padded(raw, ds, np.uint16(9000))
    assert (pdepth[:, w:] == 9.0).all() and (pcolor[:, 3 * w:] == 255).all() and (praw[:, w:] == 9000).all()
    ptr = lambda a: a.ctypes.data_as(_vp)                             # noqa: E731
    f32_tail = (cam[0], cam[1], cam[2], cam[3], ptr(E))
    ref = tc.case_k_ref(depth)
    want_state, want_cloud = ref.state(), ref.extract_point_cloud()
    assert len(want_state[0]) > 100 and len(want_cloud[0]) > 10000

    def check(volume, state, cloud, what):
        _check_state(volume, state, what)
        _check_cloud(volume.extract_arrays(), cloud, what)

    # device planes with padded rows
    for with_color in (True, False):
        d_depth, d_color = ctx.to_device(pdepth), ctx.to_device(pcolor)
        try:
            with _volume(r3d, color=with_color, stride=tc.K_STRIDE) as volume:
                ctx.call("r3d_tsdf_integrate_f32_dev", volume._h, _vp(d_depth), _vp(d_color) if with_color else None, w, h, ds, w, h, cs, 3,
                         *f32_tail)
                ctx.sync()
                if with_color:
                    check(volume, want_state, want_cloud, "case K device planes")
                else:
                    grey = tc.case_k_ref(depth, color=False)
                    check(volume, grey.state(), grey.extract_point_cloud(), "case K device planes, no colour")
        finally:
            ctx.sync()
            ctx.free(d_depth)
            ctx.free(d_color)
    # host float planes with padded rows
    with _volume(r3d, stride=tc.K_STRIDE) as volume:
        ctx.call("r3d_tsdf_integrate_f32", volume._h, ptr(pdepth), ptr(pcolor), w, h, ds, w, h, cs, 3, *f32_tail)
        check(volume, want_state, want_cloud, "case K host float planes")
    # raw uint16 depth with padded rows
    ref16 = tc.case_k_ref(tr.depth_from_u16(raw, 1000.0, 10.0))
    camera = r3d.cloud_ops.DepthCamera(cam[0], cam[1], cam[2], cam[3], 1000.0, 10.0, 0, 0)
    with _volume(r3d, stride=tc.K_STRIDE) as volume:
        ctx.call("r3d_tsdf_integrate", volume._h, ptr(praw), ptr(pcolor), w, h, ds, w, h, cs, 3, ctypes.byref(camera), ptr(E))
        check(volume, ref16.state(), ref16.extract_point_cloud(), "case K raw uint16 depth")
    # strides smaller than a row
    with _volume(r3d, stride=tc.K_STRIDE) as volume:
        for name in ("r3d_tsdf_integrate_f32", "r3d_tsdf_integrate"):
            tail = f32_tail if name == "r3d_tsdf_integrate_f32" else (ctypes.byref(camera), ptr(E))
            d = ptr(pdepth) if name == "r3d_tsdf_integrate_f32" else ptr(praw)
            assert _refused(r3d, ctx.call, name, volume._h, d, ptr(pcolor), w, h, w - 1, w, h, cs, 3, *tail) == -1
            assert _refused(r3d, ctx.call, name, volume._h, d, ptr(pcolor), w, h, ds, w, h, 3 * w - 1, 3, *tail) == -1
        d_depth, d_color = ctx.to_device(pdepth), ctx.to_device(pcolor)
        try:
            assert _refused(r3d, ctx.call, "r3d_tsdf_integrate_f32_dev", volume._h, _vp(d_depth), _vp(d_color), w, h, w - 1, w, h, cs, 3, *f32_tail) == -1
            assert _refused(r3d, ctx.call, "r3d_tsdf_integrate_f32_dev", volume._h, _vp(d_depth), _vp(d_color), w, h, ds, w, h, 3 * w - 1, 3, *f32_tail) == -1
        finally:
            ctx.sync()
            ctx.free(d_depth)
            ctx.free(d_color)
        assert len(volume) == 0 and volume.stats()["frames"] == 0 and volume.point_count() == 0


# ---- L -----------------------------------------------------------------------------------------------------------------------------
def test_case_l1_far_from_the_origin(r3d):
    states, clouds = tc.case_l1()
    idx = states[0][0]
    assert len(idx) == tc.COUNTS["l1_units"] and tuple(idx.min(0)) == tc.COUNTS["l1_lo"] and tuple(idx.max(0)) == tc.COUNTS["l1_hi"]
    assert len(clouds[0][0]) == tc.COUNTS["l1_points"]
    cam = sc.camera(64, 48)
    with _volume(r3d) as volume:
        for n, (k, pose) in enumerate(((1, tc.l1_pose()), (0, POSES_A[0]))):
            depth, color = _frame(64, 48, k)
            volume.integrate_f32(depth, color, cam, np.linalg.inv(pose))
            _check_state(volume, states[n], f"case L1 frame {n}")
            _check_cloud(volume.extract_arrays(), clouds[n], f"case L1 frame {n}")


def test_case_l2_index_limits(r3d):
    depth, color = tc.l2_frame()
    cam = sc.camera(tc.L2_W, tc.L2_H)
    ref = tr.Volume(VL, TRUNC, True, 4)
    moves = tc.l2_translations()
    with _volume(r3d) as volume:
        for axis, index, t, _ in moves:
            ref.integrate(depth, color, cam, tc.extrinsic_at(t))
            touched = np.array(ref.touched)
            assert len(touched) == tc.COUNTS["l2_units"] and (touched[:, axis] == index).all()
            volume.integrate_f32(depth, color, cam, tc.extrinsic_at(t))
            _check_state(volume, ref.state(), f"case L2 axis {axis} unit {index}")
        idx = ref.state()[0]
        assert len(idx) == 24 and idx.min() == -tc.LIMIT and idx.max() == tc.LIMIT - 1
        want = ref.extract_point_cloud()
        assert len(want[0]) == 6 * tc.COUNTS["l2_points"]
        assert volume.point_count() == len(want[0])
        _check_cloud(volume.extract_arrays(), want, "case L2")
        before = _snapshot(volume)
        for axis, index, _, beyond in moves:
            assert _refused(r3d, volume.integrate_f32, depth, color, cam, tc.extrinsic_at(beyond)) == -4, f"axis {axis}, one unit past {index}"
            assert _snapshot(volume) == before, f"the refused frame past unit {index} of axis {axis} changed the volume"
        assert volume.stats()["frames"] == 6 and volume.stats()["units"] == 24


# ---- M -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["inf", "far"])
def test_case_m_refused_on_a_live_volume(r3d, which):
    """M1 (a +inf sample) and M2 (a pose 2e5 m away) after frame 0 of case A: the refused frame leaves nothing behind"""
    cam = sc.camera(64, 48)
    states, cloud = _case_a()
    assert len(states[0][0]) == tc.COUNTS["m_units"]
    depth2, color2 = _frame(64, 48, 2)
    bad_depth, bad_pose = (tc.m_inf_depth(), POSES_A[2]) if which == "inf" else (depth2, tc.m_far_pose())
    with _volume(r3d, initial_units=8) as volume:
        depth, color = _frame(64, 48, 0)
        volume.integrate_f32(depth, color, cam, np.linalg.inv(POSES_A[0]))
        _check_state(volume, states[0], "case M frame 0")
        before = _snapshot(volume)
        assert before[0] == tc.COUNTS["m_units"] and before[1] == 1
        assert _refused(r3d, volume.integrate_f32, bad_depth, color2, cam, np.linalg.inv(bad_pose)) == -4
        assert _snapshot(volume) == before, "the refused frame changed the volume"
        for k in (1, 2):
            depth, color = _frame(64, 48, k)
            volume.integrate_f32(depth, color, cam, np.linalg.inv(POSES_A[k]))
            _check_state(volume, states[k], f"case M ({which}) frame {k} after the refusal")
        assert volume.stats()["frames"] == 3
        _check_cloud(volume.extract_arrays(), cloud, f"case M ({which})")


def test_case_m3_refused_first_frame(r3d):
    """the +inf frame into an empty pool of 8 units: the refused pass also overflowed table and pool"""
    cam = sc.camera(64, 48)
    _, cloud = _case_a()
    with _volume(r3d, initial_units=8) as volume:
        assert _refused(r3d, volume.integrate_f32, tc.m_inf_depth(), _frame(64, 48, 2)[1], cam, np.linalg.inv(POSES_A[2])) == -4
        st = volume.stats()
        assert len(volume) == 0 and st["frames"] == 0 and volume.point_count() == 0 and len(volume.debug_units()[0]) == 0
        _run_case_a(r3d, volume)
        assert volume.stats()["frames"] == 3
        _check_cloud(volume.extract_arrays(), cloud, "case M3")


# ---- N -----------------------------------------------------------------------------------------------------------------------------
def test_case_n_nan_is_no_sample(r3d):
    cam = sc.camera(64, 48)
    nan, zero, valid = tc.n_depths()
    (s_nan, c_nan), _ = tc.case_n()
    assert valid == tc.COUNTS["n_valid"] and len(s_nan[0]) == tc.COUNTS["n_units"] and len(c_nan[0]) == tc.COUNTS["n_points"]
    color = _frame(64, 48, 1)[1]
    outs = []
    for name, depth in (("NaN", nan), ("zero", zero)):
        with _volume(r3d) as volume:
            volume.integrate_f32(depth, color, cam, np.linalg.inv(POSES_A[1]))
            _check_state(volume, s_nan, f"case N, {name} patch")
            _check_cloud(volume.extract_arrays(), c_nan, f"case N, {name} patch")
            outs.append([a.tobytes() for a in volume.debug_units()])
    assert outs[0] == outs[1]


# ---- P -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(3))
def test_case_p_tiny_images(r3d, case):
    w, h, stride, cam = tc.P_CASES[case]
    depth, color = tc.p_frame(w, h)
    ref = tr.Volume(VL, TRUNC, True, stride)
    ref.integrate(depth, color, cam, np.eye(4))
    idx, _, wt, _ = ref.state()
    want = ref.extract_point_cloud()
    assert (len(idx), int((wt != 0).sum()), len(want[0])) == tc.COUNTS["p"][case]
    with _volume(r3d, stride=stride) as volume:
        volume.integrate_f32(depth, color, cam, np.eye(4))
        _check_state(volume, ref.state(), f"case P {w} x {h}")
        _check_cloud(volume.extract_arrays(), want, f"case P {w} x {h}")
