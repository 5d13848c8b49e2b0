"""Inputs of the TSDF edge cases J to P, shared by tests/test_tsdf_ref.py (the restatement's two forms agree there and the
counts are pinned) and tests/test_tsdf_edges_gpu.py (the device against the restatement).  Every function returns plain numpy
inputs; the restatement runs that take seconds are computed once and must be left unchanged by their users.

The counts in COUNTS are the restatement's.  They are what shows that a case still reaches its regime (more than 512 units, a
unit index of exactly +-2^20, new units in the refused frame): an input changed without rechecking them fails on the CPU."""
import functools

import numpy as np

from tests import rgbd_scene as sc
from tests import tsdf_ref as tr
from tests.test_tsdf_gpu import POSES_A, TRUNC, VL, _frame

UL = VL * tr.R
LIMIT = 1 << 20

COUNTS = dict(
    j_units=(517, 576), j_points=117221,
    l1_units=193, l1_lo=(-6256, 12495, 3133), l1_hi=(-6245, 12503, 3135), l1_points=29378,
    l2_weighted=(122, 110, 104), l2_units=4, l2_points=4,
    m_units=194,
    n_valid=222, n_units=187, n_points=27336,
    p=((8, 88, 4), (8, 7738, 570), (4, 6725, 400)),
)


def state_copy(vol):
    return tuple(None if a is None else a.copy() for a in vol.state())


# ---- J: past 256 and 512 units ---------------------------------------------------------------------------------------------------
J_VL, J_TRUNC = 0.005, 0.02


@functools.lru_cache(maxsize=None)
def case_j():
    """-> states after frames 0 and 1 of case A in a volume of 5 mm voxels, and the cloud (read-only; about 2 s)"""
    vol = tr.Volume(J_VL, J_TRUNC, True, 4)
    cam = sc.camera(64, 48)
    states = []
    for k in (0, 1):
        depth, color = _frame(64, 48, k)
        vol.integrate(depth, color, cam, np.linalg.inv(POSES_A[k]))
        states.append(state_copy(vol))
    return states, vol.extract_point_cloud()


# ---- K: padded rows --------------------------------------------------------------------------------------------------------------
K_W, K_H, K_STRIDE = 50, 37, 3
K_DPAD, K_CPAD = 5, 7


@functools.lru_cache(maxsize=None)
def case_k_images():
    """-> depth float32 [37,50], colour uint8 [37,50,3] with three different channels (case C's), read-only"""
    inten, depth = sc.render(K_W, K_H, sc.TRUTH, sc.HOLES)
    color = np.ascontiguousarray(np.stack([(inten * 255).astype(np.uint8), (inten * 100).astype(np.uint8), (inten * 30).astype(np.uint8)], -1))
    return depth, color


def padded(plane, row_elems, fill):
    """-> a [rows, row_elems] buffer whose first columns hold `plane` ([rows, n]) and whose padding holds `fill`"""
    rows, n = plane.shape
    out = np.full((rows, row_elems), fill, plane.dtype)
    out[:, :n] = plane
    return out


def case_k_ref(depth, color=True):
    depth_img, color_img = case_k_images()
    vol = tr.Volume(VL, TRUNC, color, K_STRIDE)
    vol.integrate(depth, color_img if color else None, sc.camera(K_W, K_H), np.linalg.inv(sc.TRUTH))
    return vol


# ---- L: large and extreme unit indices -------------------------------------------------------------------------------------------
def l1_pose():
    pose = POSES_A[1].copy()
    pose[:3, 3] += (-1000.0, 2000.0, 500.0)
    return pose


@functools.lru_cache(maxsize=None)
def case_l1():
    """-> states and clouds after frame 1 at the far pose and after frame 0 at POSES_A[0] in the same volume (read-only)"""
    vol = tr.Volume(VL, TRUNC, True, 4)
    cam = sc.camera(64, 48)
    states, clouds = [], []
    for k, pose in ((1, l1_pose()), (0, POSES_A[0])):
        depth, color = _frame(64, 48, k)
        vol.integrate(depth, color, cam, np.linalg.inv(pose))
        states.append(state_copy(vol))
        clouds.append(vol.extract_point_cloud())
    return states, clouds


L2_W, L2_H, L2_DEPTH = 32, 24, 0.03


def l2_frame():
    return np.full((L2_H, L2_W), L2_DEPTH, np.float32), np.full((L2_H, L2_W, 3), 77, np.uint8)


def l2_translations():
    """-> [(axis, unit index the frame lands in, camera position t, the same moved one unit length outward)] x 6"""
    out = []
    for axis in range(3):
        for index, comp, step in ((LIMIT - 1, (LIMIT - 1) * UL + UL / 2, UL), (-LIMIT, -LIMIT * UL + UL / 2, -UL)):
            t = np.zeros(3)
            t[axis] = comp - (L2_DEPTH if axis == 2 else 0.0)
            beyond = t.copy()
            beyond[axis] += step
            out.append((axis, index, t, beyond))
    return out


def extrinsic_at(t):
    """[I | -t]: a camera at t that looks along +z"""
    E = np.eye(4)
    E[:3, 3] = -np.asarray(t, dtype=np.float64)
    return E


# ---- M: a refused frame on a live volume -----------------------------------------------------------------------------------------
M_PIXEL = (8, 12)          # row, column: both multiples of the stride 4, so the touch pass reads the sample


def m_inf_depth():
    depth = _frame(64, 48, 2)[0].copy()
    depth[M_PIXEL] = np.inf
    return depth


def m_far_pose():
    pose = POSES_A[2].copy()
    pose[0, 3] += 2e5          # 2e5 m / 0.16 m = 1.25e6 units > 2^20: every sample is out of range
    return pose


# ---- N: NaN means no sample ------------------------------------------------------------------------------------------------------
N_ROWS, N_COLS = slice(8, 21), slice(12, 30)


def n_depths():
    """-> frame 1 of case A with the patch NaN, the same with the patch 0, the number of valid pixels the patch had"""
    depth = _frame(64, 48, 1)[0]
    nan, zero = depth.copy(), depth.copy()
    nan[N_ROWS, N_COLS] = np.nan
    zero[N_ROWS, N_COLS] = 0
    return nan, zero, int((depth[N_ROWS, N_COLS] > 0).sum())


@functools.lru_cache(maxsize=None)
def case_n():
    """-> (state, cloud) of the NaN image and of the zero image (read-only)"""
    out = []
    for depth in n_depths()[:2]:
        vol = tr.Volume(VL, TRUNC, True, 4)
        vol.integrate(depth, _frame(64, 48, 1)[1], sc.camera(64, 48), np.linalg.inv(POSES_A[1]))
        out.append((state_copy(vol), vol.extract_point_cloud()))
    return tuple(out)


# ---- P: tiny images --------------------------------------------------------------------------------------------------------------
P_CASES = ((1, 1, 1, (20.0, 20.0, 0.0, 0.0)), (5, 3, 4, (4.0, 4.0, 2.0, 1.0)), (3, 2, 4, (3.0, 3.0, 1.0, 0.5)))     # w, h, stride, camera


def p_frame(w, h):
    return np.full((h, w), 0.5, np.float32), np.arange(h * w * 3, dtype=np.uint8).reshape(h, w, 3)
