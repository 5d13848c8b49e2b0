"""numpy-facing wrappers of the point-cloud entry points of the C ABI (include/r3d.h).  No CPU fallback."""
import ctypes

import numpy as np

from . import _lib

_vp = ctypes.c_void_p
_dp = ctypes.POINTER(ctypes.c_double)

_lib.register({
    "r3d_voxel_downsample": ([_vp, _vp, _vp, _vp, ctypes.c_int64, ctypes.c_double, _vp, _vp, _vp,
                              ctypes.POINTER(ctypes.c_int64)], ctypes.c_int),
    "r3d_voxel_downsample_tensor": ([_vp, _vp, _vp, _vp, ctypes.c_int64, ctypes.c_double, _vp, _vp, _vp,
                                     ctypes.POINTER(ctypes.c_int64)], ctypes.c_int),
    "r3d_estimate_normals": ([_vp, _vp, ctypes.c_int64, ctypes.c_double, ctypes.c_int32, _vp, _vp], ctypes.c_int),
    "r3d_neighbor_score": ([_vp, _vp, ctypes.c_int64, ctypes.c_int32, ctypes.c_double, _vp], ctypes.c_int),
    "r3d_reproject_disparity": ([_vp, _vp, ctypes.c_int32, ctypes.c_int32, _vp, ctypes.c_int32, _vp, _vp,
                                 ctypes.POINTER(ctypes.c_int64)], ctypes.c_int),
    "r3d_disparity_to_cloud_dev": ([_vp, _vp, ctypes.c_int32, ctypes.c_int32, _vp, ctypes.c_int32, ctypes.c_double, _vp,
                                    ctypes.c_double, ctypes.c_double, ctypes.c_int32, ctypes.c_int64, _vp, _vp,
                                    ctypes.POINTER(ctypes.c_int64)], ctypes.c_int),
    "r3d_disparity_to_cloud_color_dev": ([_vp, _vp, ctypes.c_int32, ctypes.c_int32, _vp, ctypes.c_int32, ctypes.c_double, _vp,
                                          ctypes.c_double, ctypes.c_double, ctypes.c_int32, _vp, ctypes.c_int32, ctypes.c_int32,
                                          ctypes.c_int32, ctypes.c_int64, _vp, _vp, _vp, ctypes.POINTER(ctypes.c_int64)], ctypes.c_int),
    "r3d_knn_graph": ([_vp, _vp, ctypes.c_int64, ctypes.c_int32, ctypes.c_double, _vp, _vp], ctypes.c_int),
    "r3d_orient_normals": ([_vp, _vp, ctypes.c_int64, ctypes.c_int32, _vp], ctypes.c_int),
    "r3d_orient_normals_graph": ([_vp, _vp, ctypes.c_int64, ctypes.c_int32, _vp, ctypes.c_int64, _vp], ctypes.c_int),
    "r3d_transform_points": ([_vp, _vp, ctypes.c_int64, _vp, ctypes.c_int32, _vp], ctypes.c_int),
    "r3d_icp": ([_vp, ctypes.POINTER(_lib.IcpParams), _vp, ctypes.c_int64, _vp, _vp, ctypes.c_int64, _vp, _vp, _vp,
                 ctypes.POINTER(_lib.IcpStats)], ctypes.c_int),
})

P2P, P2PLANE, GICP = 0, 1, 2
COLORED = 3     # registration_colored / registration_colored_device only: r3d_icp itself refuses it

_lib.register({
    "r3d_color_gradients": ([_vp, _vp, _vp, _vp, ctypes.c_int64, ctypes.c_double, ctypes.c_int32, _vp, _vp], ctypes.c_int),
    "r3d_icp_colored": ([_vp, ctypes.POINTER(_lib.ColoredIcpParams), _vp, _vp, ctypes.c_int64, _vp, _vp, _vp, ctypes.c_int64, _vp, _vp,
                         ctypes.POINTER(_lib.IcpStats)], ctypes.c_int),
    "r3d_icp_colored_dev": ([_vp, ctypes.POINTER(_lib.ColoredIcpParams), _vp, _vp, ctypes.c_int64, _vp, _vp, _vp, ctypes.c_int64, _vp, _vp,
                             ctypes.POINTER(_lib.IcpStats)], ctypes.c_int),
})

FPFH_DIM = 33
_lib.register({
    "r3d_compute_fpfh": ([_vp, _vp, _vp, ctypes.c_int64, ctypes.c_double, ctypes.c_int32, _vp, _vp], ctypes.c_int),
    "r3d_compute_fpfh_dev": ([_vp, _vp, _vp, ctypes.c_int64, ctypes.c_double, ctypes.c_int32, _vp, _vp], ctypes.c_int),
    "r3d_fpfh_from_spfh": ([_vp, _vp, ctypes.c_int64, ctypes.c_double, ctypes.c_int32, _vp, _vp], ctypes.c_int),
    "r3d_match_features": ([_vp, _vp, ctypes.c_int64, _vp, ctypes.c_int64, ctypes.c_int32, _vp, _vp], ctypes.c_int),
    "r3d_match_features_dev": ([_vp, _vp, ctypes.c_int64, _vp, ctypes.c_int64, ctypes.c_int32, _vp, _vp], ctypes.c_int),
    "r3d_debug_fpfh_stages": ([_vp, _vp, _vp, ctypes.c_int64, ctypes.c_double, ctypes.c_int32, _vp, ctypes.POINTER(ctypes.c_float)], ctypes.c_int),
})


class RansacParams(ctypes.Structure):
    """r3d_ransac_params"""
    _fields_ = [("max_correspondence_distance", ctypes.c_double), ("edge_length_similarity", ctypes.c_double),
                ("checker_distance", ctypes.c_double), ("confidence", ctypes.c_double), ("max_iteration", ctypes.c_int64),
                ("seed", ctypes.c_uint64), ("ransac_n", ctypes.c_int32), ("batch", ctypes.c_int32)]


class RansacStats(ctypes.Structure):
    """r3d_ransac_stats"""
    _fields_ = [("fitness", ctypes.c_double), ("inlier_rmse", ctypes.c_double), ("iterations", ctypes.c_int64),
                ("validated", ctypes.c_int64), ("best_hypothesis", ctypes.c_int64), ("inliers", ctypes.c_int64),
                ("setup_ms", ctypes.c_double), ("loop_ms", ctypes.c_double)]


_ransac_sig = ([_vp, ctypes.POINTER(RansacParams), _vp, ctypes.c_int64, _vp, ctypes.c_int64, _vp, ctypes.c_int64, _vp, _vp,
                ctypes.POINTER(RansacStats)], ctypes.c_int)
_lib.register({
    "r3d_ransac_correspondence": _ransac_sig,
    "r3d_ransac_correspondence_dev": _ransac_sig,
    "r3d_debug_ransac_hypotheses": ([_vp, ctypes.POINTER(RansacParams), _vp, ctypes.c_int64, _vp, ctypes.c_int64, _vp, ctypes.c_int64,
                                     ctypes.c_int64, ctypes.c_int64, _vp, _vp, _vp, _vp, _vp], ctypes.c_int),
})

class FgrParams(ctypes.Structure):
    """r3d_fgr_params"""
    _fields_ = [("division_factor", ctypes.c_double), ("maximum_correspondence_distance", ctypes.c_double),
                ("tuple_scale", ctypes.c_double), ("seed", ctypes.c_uint64), ("iteration_number", ctypes.c_int32),
                ("maximum_tuple_count", ctypes.c_int32), ("use_absolute_scale", ctypes.c_int32), ("decrease_mu", ctypes.c_int32),
                ("tuple_test", ctypes.c_int32), ("batch", ctypes.c_int32)]


class FgrStats(ctypes.Structure):
    """r3d_fgr_stats"""
    _fields_ = [(n, ctypes.c_double) for n in ("fitness", "inlier_rmse", "scale_global", "scale_start", "final_par", "setup_ms",
                                               "loop_ms")] + \
               [(n, ctypes.c_int64) for n in ("correspondences", "matched", "trials", "tuples", "pairs")]


_fgr_corr_sig = ([_vp, ctypes.POINTER(FgrParams), _vp, ctypes.c_int64, _vp, ctypes.c_int64, _vp, ctypes.c_int64, _vp,
                  ctypes.POINTER(FgrStats)], ctypes.c_int)
_fgr_feat_sig = ([_vp, ctypes.POINTER(FgrParams), _vp, ctypes.c_int64, _vp, ctypes.c_int64, _vp, _vp, ctypes.c_int32, _vp,
                  ctypes.POINTER(FgrStats)], ctypes.c_int)
_lib.register({
    "r3d_fgr_correspondence": _fgr_corr_sig,
    "r3d_fgr_correspondence_dev": _fgr_corr_sig,
    "r3d_fgr_feature_matching": _fgr_feat_sig,
    "r3d_fgr_feature_matching_dev": _fgr_feat_sig,
    "r3d_debug_fgr_tuples": ([_vp, ctypes.POINTER(FgrParams), _vp, ctypes.c_int64, _vp, ctypes.c_int64, _vp, ctypes.c_int64, ctypes.c_int64,
                              ctypes.c_int64, _vp, _vp], ctypes.c_int),
    "r3d_debug_fgr_optimize": ([_vp, ctypes.POINTER(FgrParams), _vp, ctypes.c_int64, _vp, ctypes.c_int64, _vp, ctypes.c_int64, _vp, _vp],
                               ctypes.c_int),
})

_lib.register({
    "r3d_debug_sort_by_cell": ([_vp, _vp, ctypes.c_int64, _vp, ctypes.c_double, _vp, ctypes.c_int32, ctypes.c_int32, _vp, _vp], ctypes.c_int),
    "r3d_debug_exclusive_scan": ([_vp, _vp, ctypes.c_int64, ctypes.c_int32, _vp], ctypes.c_int),
    "r3d_debug_icp_correspondences": ([_vp, _vp, ctypes.c_int64, _vp, ctypes.c_int64, ctypes.c_double, _vp, _vp, _vp], ctypes.c_int),
    "r3d_debug_icp_sums": ([_vp, ctypes.POINTER(_lib.IcpParams), _vp, ctypes.c_int64, _vp, _vp, ctypes.c_int64, _vp, _vp, _vp, _vp],
                           ctypes.c_int),
    "r3d_debug_icp_sums_colored": ([_vp, ctypes.POINTER(_lib.ColoredIcpParams), _vp, _vp, ctypes.c_int64, _vp, _vp, _vp, ctypes.c_int64, _vp,
                                    _vp, _vp], ctypes.c_int),
})


def debug_exclusive_scan(values, maximum=False, ctx=None):
    """r3d_debug_exclusive_scan: exclusive prefix sum (or running maximum) of int32 values on the device."""
    ctx = ctx or _lib.default_context()
    v = np.ascontiguousarray(values, dtype=np.int32)
    out = np.empty_like(v)
    ctx.call("r3d_debug_exclusive_scan", v.ctypes.data_as(_vp), len(v), int(bool(maximum)), out.ctypes.data_as(_vp))
    return out


def debug_sort_by_cell(points, origin, cell, dims, key_order, impl=0, ctx=None):
    """r3d_debug_sort_by_cell: (idx, keys) of the stable (cell key, index) sort; impl 0 = counting sort, 1 = radix fallback."""
    ctx = ctx or _lib.default_context()
    p = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
    org = np.ascontiguousarray(origin, dtype=np.float64)
    d = np.ascontiguousarray(dims, dtype=np.int32)
    idx = np.empty(len(p), np.int32)
    keys = np.empty(len(p), np.uint64)
    ctx.call("r3d_debug_sort_by_cell", p.ctypes.data_as(_vp), len(p), org.ctypes.data_as(_vp), float(cell), d.ctypes.data_as(_vp), int(key_order),
             int(impl), idx.ctypes.data_as(_vp), keys.ctypes.data_as(_vp))
    return idx, keys


def debug_icp_correspondences(source, target, max_correspondence_distance, T=None, want_d2=True, ctx=None):
    """r3d_debug_icp_correspondences: (corr [ns] int32, d2 [ns]) of one evaluation of the registration's search at pose T:
    corr[i] is the index of the target nearest to T * source[i], -1 where none lies within the distance (d2 = 1e300)."""
    ctx = ctx or _lib.default_context()
    s = np.ascontiguousarray(source, dtype=np.float64).reshape(-1, 3)
    t = np.ascontiguousarray(target, dtype=np.float64).reshape(-1, 3)
    T0 = None if T is None else np.ascontiguousarray(T, dtype=np.float64).reshape(4, 4)
    corr = np.empty(len(s), np.int32)
    d2 = np.empty(len(s)) if want_d2 else None
    ctx.call("r3d_debug_icp_correspondences", s.ctypes.data_as(_vp), len(s), t.ctypes.data_as(_vp), len(t), float(max_correspondence_distance),
             None if T0 is None else T0.ctypes.data_as(_vp), corr.ctypes.data_as(_vp), None if d2 is None else d2.ctypes.data_as(_vp))
    return corr, d2


def debug_icp_sums(source, target, max_distance, mode, T=None, source_normals=None, target_normals=None, gicp_epsilon=0.0, ctx=None):
    """r3d_debug_icp_sums: (sums [29], origin [3]) of one evaluation of the registration loop in mode 0, 1 or 2 at pose T, as the
    device reduces them for its step.  The slots' meaning, and the origin the point-to-point slots are relative to: include/r3d.h."""
    ctx = ctx or _lib.default_context()
    s, t, sn, tn = _c(source), _c(target), _c(source_normals), _c(target_normals)
    T0 = None if T is None else np.ascontiguousarray(T, dtype=np.float64).reshape(4, 4)
    prm = _lib.IcpParams(int(mode), 0, float(max_distance), 0.0, 0.0, float(gicp_epsilon))
    sums, origin = np.empty(29), np.empty(3)
    ctx.call("r3d_debug_icp_sums", ctypes.byref(prm), _ptr(s), len(s), _ptr(sn), _ptr(t), len(t), _ptr(tn), _ptr(T0), _ptr(sums), _ptr(origin))
    return sums, origin


class AlignParams(ctypes.Structure):
    _fields_ = [("icp", _lib.IcpParams), ("voxel_size", ctypes.c_double), ("normal_radius", ctypes.c_double),
                ("normal_max_nn", ctypes.c_int32), ("reserved", ctypes.c_int32)]


_lib.register({
    "r3d_align_point_clouds": ([_vp, ctypes.POINTER(AlignParams), _vp, _vp, ctypes.c_int64, _vp, ctypes.c_int64, _vp, _vp, _vp,
                                _vp, ctypes.POINTER(ctypes.c_int64), _vp, ctypes.POINTER(_lib.IcpStats)], ctypes.c_int),
})


_i64p = ctypes.POINTER(ctypes.c_int64)


class DepthCamera(ctypes.Structure):
    """r3d_depth_camera: pinhole intrinsics (camera_intrinsic.json) + the depth conversion of create_from_rgbd_image."""
    _fields_ = [("fx", ctypes.c_double), ("fy", ctypes.c_double), ("ppx", ctypes.c_double), ("ppy", ctypes.c_double),
                ("depth_scale", ctypes.c_double), ("depth_trunc", ctypes.c_double), ("flip_yz", ctypes.c_int32),
                ("reserved", ctypes.c_int32)]


# test/check84.py:158 passes depth_scale = 1.0 / sensor depth scale, the sensor value being the float32 0.001
DEPTH_SCALE_REALSENSE = float(np.float32(1.0) / np.float32(0.001))


def depth_camera(intrinsics, depth_scale=DEPTH_SCALE_REALSENSE, depth_trunc=3.0, flip=True):
    """intrinsics: dict with fx / fy / ppx / ppy (the reference's camera_intrinsic.json) or a 3x3 matrix."""
    if isinstance(intrinsics, dict):
        fx, fy, ppx, ppy = (float(intrinsics[k]) for k in ("fx", "fy", "ppx", "ppy"))
    else:
        K = np.asarray(intrinsics, dtype=np.float64).reshape(3, 3)
        fx, fy, ppx, ppy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    return DepthCamera(fx, fy, ppx, ppy, float(depth_scale), float(depth_trunc), int(bool(flip)), 0)


def _depth_args(depth, color):
    d = np.ascontiguousarray(depth, dtype=np.uint16)
    if d.ndim != 2:
        raise ValueError("depth image must be 2-D uint16")
    c = None
    if color is not None:
        c = np.ascontiguousarray(color, dtype=np.uint8)
        if c.shape != d.shape + (3,):
            raise ValueError(f"colour image {c.shape} does not match the depth image {d.shape} (3 channels expected)")
    return d, c


_lib.register({
    "r3d_backproject_depth": ([_vp, _vp, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(DepthCamera), _vp, ctypes.c_int32,
                               _vp, _vp, _vp, _i64p], ctypes.c_int),
    "r3d_model_append_depth": ([_vp, _vp, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(DepthCamera), _vp, ctypes.c_int32,
                                _i64p], ctypes.c_int),
    "r3d_model_align_append_depth": ([_vp, ctypes.POINTER(AlignParams), _vp, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                      ctypes.POINTER(DepthCamera), _vp, ctypes.c_int32, _vp, ctypes.POINTER(_lib.IcpStats), _i64p, _i64p],
                                     ctypes.c_int),
    "r3d_model_create": ([_vp, ctypes.POINTER(_vp)], ctypes.c_int),
    "r3d_model_destroy": ([_vp], None),
    "r3d_model_clear": ([_vp], ctypes.c_int),
    "r3d_model_size": ([_vp, _i64p, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32)], ctypes.c_int),
    "r3d_model_voxel_table_stats": ([_vp, _i64p, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32)], ctypes.c_int),
    "r3d_model_debug_voxel_table": ([_vp, ctypes.c_double, ctypes.c_int64, _vp, _vp, _vp, _vp, _vp, _i64p, ctypes.POINTER(ctypes.c_int32)],
                                    ctypes.c_int),
    "r3d_model_debug_fail_table_step": ([_vp, ctypes.c_int32], ctypes.c_int),
    "r3d_model_append": ([_vp, _vp, _vp, _vp, ctypes.c_int64], ctypes.c_int),
    "r3d_model_align_append": ([_vp, ctypes.POINTER(AlignParams), _vp, _vp, ctypes.c_int64, _vp, ctypes.POINTER(_lib.IcpStats), _i64p],
                               ctypes.c_int),
    "r3d_model_register_append": ([_vp, ctypes.POINTER(_lib.IcpParams), _vp, _vp, _vp, ctypes.c_int64, _vp,
                                   ctypes.POINTER(_lib.IcpStats)], ctypes.c_int),
    "r3d_model_estimate_normals": ([_vp, ctypes.c_double, ctypes.c_int32], ctypes.c_int),
    "r3d_model_download": ([_vp, _vp, _vp, _vp], ctypes.c_int),
    "r3d_disparity_to_cloud_resident": ([_vp, _vp, ctypes.c_int32, ctypes.c_int32, _vp, ctypes.c_int32, ctypes.c_double, _vp,
                                         ctypes.c_double, ctypes.c_double, ctypes.c_int32, ctypes.c_int64, _vp, _vp, _i64p], ctypes.c_int),
    "r3d_disparity_to_cloud_color_resident": ([_vp, _vp, ctypes.c_int32, ctypes.c_int32, _vp, ctypes.c_int32, ctypes.c_double, _vp,
                                               ctypes.c_double, ctypes.c_double, ctypes.c_int32, _vp, ctypes.c_int32, ctypes.c_int32,
                                               ctypes.c_int32, ctypes.c_int64, _vp, _vp, _vp, _i64p], ctypes.c_int),
    "r3d_icp_dev": ([_vp, ctypes.POINTER(_lib.IcpParams), _vp, ctypes.c_int64, _vp, _vp, ctypes.c_int64, _vp, _vp, _vp,
                     ctypes.POINTER(_lib.IcpStats)], ctypes.c_int),
    "r3d_transform_points_dev": ([_vp, _vp, ctypes.c_int64, _vp, ctypes.c_int32, _vp], ctypes.c_int),
    "r3d_transform_blocks_dev": ([_vp, ctypes.c_int32, _vp, _vp, _vp, _vp, _vp], ctypes.c_int),
})


def _c(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float64).reshape(-1, 3)


_ptr = _lib.ptr


def voxel_down_sample(points, voxel, colors=None, normals=None, ctx=None, tensor=False):
    """Legacy voxel_down_sample (grid origin min_bound - voxel/2, float64 means); tensor=True: the o3d.t method on a Float32
    cloud (origin 0, float32 keys and means; pointcloud_processing.py:27).  Voxels come out in lexicographic key order."""
    ctx = ctx or _lib.default_context()
    p, c, n = _c(points), _c(colors), _c(normals)
    N = len(p)
    if N == 0:
        return p, c, n
    op = np.empty((N, 3))
    oc = np.empty((N, 3)) if c is not None else None
    on = np.empty((N, 3)) if n is not None else None
    m = ctypes.c_int64()
    ctx.call("r3d_voxel_downsample_tensor" if tensor else "r3d_voxel_downsample", _ptr(p), _ptr(c), _ptr(n), N, float(voxel),
             _ptr(op), _ptr(oc), _ptr(on), ctypes.byref(m))
    m = m.value
    return op[:m].copy(), (oc[:m].copy() if oc is not None else None), (on[:m].copy() if on is not None else None)


def estimate_normals(points, radius, max_nn, prev_normals=None, ctx=None):
    """radius None or <= 0 -> pure kNN (KDTreeSearchParamKNN)."""
    ctx = ctx or _lib.default_context()
    p, pn = _c(points), _c(prev_normals)
    out = np.empty_like(p)
    if len(p) == 0:                      # Open3D returns the empty cloud unchanged
        return out
    ctx.call("r3d_estimate_normals", _ptr(p), len(p), float(radius) if radius else -1.0, int(max_nn), _ptr(pn), _ptr(out))
    return out


def neighbor_score(points, k=0, count_radius=0.0, ctx=None):
    ctx = ctx or _lib.default_context()
    p = _c(points)
    out = np.empty(len(p))
    ctx.call("r3d_neighbor_score", _ptr(p), len(p), int(k), float(count_radius), out.ctypes.data_as(_vp))
    return out


def reproject_disparity(disp, Q, min_disparity=0, want_pixels=False, ctx=None):
    """disp: int16 [H,W] (x16, as StereoSGBM.compute returns it); Q: 4x4.  Returns points [M,3] (and pixel indices)."""
    ctx = ctx or _lib.default_context()
    d = np.ascontiguousarray(disp, dtype=np.int16)
    H, W = d.shape
    Q = np.ascontiguousarray(Q, dtype=np.float64).reshape(4, 4)
    out = np.empty((H * W, 3))
    pix = np.empty(H * W, np.int32) if want_pixels else None
    m = ctypes.c_int64()
    ctx.call("r3d_reproject_disparity", d.ctypes.data_as(_vp), W, H, _ptr(Q), int(min_disparity) * 16, _ptr(out),
             pix.ctypes.data_as(_vp) if want_pixels else None, ctypes.byref(m))
    out = out[:m.value].copy()
    return (out, pix[:m.value].copy()) if want_pixels else out


def _color_args(d_color, width, color_stride, color_channels, color_order):
    """The four colour arguments of the r3d_disparity_to_cloud_color_* entry points (the library checks channels and stride)."""
    if color_order not in ("bgr", "rgb"):
        raise ValueError(f"color_order must be 'bgr' or 'rgb', got {color_order!r}")
    cn = int(color_channels)
    return _vp(d_color), int(color_stride) if color_stride is not None else int(width) * cn, cn, int(color_order == "bgr")


def disparity_to_cloud_device(d_disp, width, height, Q, min_disparity=0, max_depth=None, pose=None, voxel=0.01,
                              normal_radius=None, max_nn=30, capacity=None, ctx=None, d_color=None, color_stride=None,
                              color_channels=3, color_order="bgr"):
    """Device-resident disparity -> cloud chain (r3d_disparity_to_cloud_dev): d_disp is the device pointer (int) of an
    int16 [height,width] map as written by StereoSGBM.compute_device.  Returns (points [M,3], normals [M,3] or None).
    d_color (device pointer of a uint8 image of the map's size; color_stride: bytes per row, default width * color_channels;
    color_channels 1 or 3; color_order "bgr" as cv2 stores it, or "rgb") colours the cloud from that image
    (r3d_disparity_to_cloud_color_dev): returns (points, normals, colors [M,3] in r, g, b order, byte / 255)."""
    ctx = ctx or _lib.default_context()
    Q = np.ascontiguousarray(Q, dtype=np.float64).reshape(4, 4)
    P = None if pose is None else np.ascontiguousarray(pose, dtype=np.float64).reshape(4, 4)
    cap = int(capacity) if capacity is not None else int(width) * int(height)
    pts = np.empty((cap, 3))
    nrm = np.empty((cap, 3)) if max_nn and max_nn > 0 else None
    m = ctypes.c_int64()
    head = (_vp(d_disp), int(width), int(height), _ptr(Q), int(min_disparity) * 16, float(max_depth) if max_depth else -1.0, _ptr(P),
            float(voxel) if voxel else -1.0, float(normal_radius) if normal_radius else -1.0, int(max_nn) if max_nn else 0)
    if d_color is None:
        ctx.call("r3d_disparity_to_cloud_dev", *head, cap, _ptr(pts), _ptr(nrm), ctypes.byref(m))
        return pts[:m.value].copy(), (nrm[:m.value].copy() if nrm is not None else None)
    col = np.empty((cap, 3))
    ctx.call("r3d_disparity_to_cloud_color_dev", *head, *_color_args(d_color, width, color_stride, color_channels, color_order), cap,
             _ptr(pts), _ptr(nrm), _ptr(col), ctypes.byref(m))
    return pts[:m.value].copy(), (nrm[:m.value].copy() if nrm is not None else None), col[:m.value].copy()


def knn_graph(points, k, radius=0.0, want_d2=True, ctx=None):
    ctx = ctx or _lib.default_context()
    p = _c(points)
    k = int(min(k, len(p)))
    nbr = np.empty((len(p), k), np.int32)
    d2 = np.empty((len(p), k)) if want_d2 else None
    ctx.call("r3d_knn_graph", _ptr(p), len(p), k, float(radius), nbr.ctypes.data_as(_vp), _ptr(d2))
    return nbr, d2


def orient_normals(points, normals, k=100, delaunay_edges=None, ctx=None):
    """orient_normals_consistent_tangent_plane(k): returns the re-oriented copy of `normals`.  delaunay_edges ([m,2] int):
    edges of the cloud's Delaunay tetrahedralisation -> the exact Open3D graph (r3d_orient_normals_graph); None -> the
    k-NN-graph-only variant (r3d_orient_normals, a documented deviation)."""
    ctx = ctx or _lib.default_context()
    p = _c(points)
    n = np.ascontiguousarray(normals, dtype=np.float64).reshape(-1, 3).copy()
    if len(p) == 0:
        return n
    if delaunay_edges is None:
        ctx.call("r3d_orient_normals", _ptr(p), len(p), int(k), _ptr(n))
    else:
        e = np.ascontiguousarray(delaunay_edges, dtype=np.int32).reshape(-1, 2)
        ctx.call("r3d_orient_normals_graph", _ptr(p), len(p), int(k), e.ctypes.data_as(_vp), len(e), _ptr(n))
    return n


def statistical_outlier_mask(points, nb_neighbors, std_ratio, ctx=None):
    """remove_statistical_outlier(nb_neighbors, std_ratio) (pointcloud_processing.py:35) [recalled RemoveStatisticalOutliers]:
    score a_i = mean distance to the k nearest (self included); the cloud mean sums the scores > 0 and divides by the number
    of points, the deviation sums over scores > 0 and divides by n - 1; keep iff 0 < a_i < mean + ratio * std.  Scores of 0
    need >= k coincident points; without them this is the plain mean / std(ddof=1) rule the recorded PLY files verify."""
    n = len(_c(points))
    if n == 0:
        return np.zeros(0, bool)
    a = neighbor_score(points, k=min(int(nb_neighbors), n), ctx=ctx)
    pos = a > 0
    mean = a[pos].sum() / n
    std = np.sqrt(((a[pos] - mean) ** 2).sum() / (n - 1)) if n > 1 else 0.0
    return pos & (a < mean + std_ratio * std)


def radius_outlier_mask(points, nb_points, radius, ctx=None):
    if len(_c(points)) == 0:
        return np.zeros(0, bool)
    return neighbor_score(points, count_radius=radius, ctx=ctx) > nb_points


def transform_points(points, T, rotate_only=False, ctx=None):
    ctx = ctx or _lib.default_context()
    p = _c(points)
    T = np.ascontiguousarray(T, dtype=np.float64).reshape(4, 4)
    out = np.empty_like(p)
    ctx.call("r3d_transform_points", _ptr(p), len(p), _ptr(T), int(bool(rotate_only)), _ptr(out))
    return out


def registration(source, target, max_correspondence_distance, init=None, mode=P2P, max_iteration=30,
                 relative_fitness=1e-6, relative_rmse=1e-6, source_normals=None, target_normals=None,
                 gicp_epsilon=1e-3, ctx=None):
    """registration_icp / registration_generalized_icp.  Returns dict(T, fitness, inlier_rmse, iterations, ...)."""
    ctx = ctx or _lib.default_context()
    s, t, sn, tn = _c(source), _c(target), _c(source_normals), _c(target_normals)
    T0 = None if init is None else np.ascontiguousarray(init, dtype=np.float64).reshape(4, 4)
    T = np.empty((4, 4))
    prm = _lib.IcpParams(int(mode), int(max_iteration), float(max_correspondence_distance), float(relative_fitness),
                         float(relative_rmse), float(gicp_epsilon))
    st = _lib.IcpStats()
    ctx.call("r3d_icp", ctypes.byref(prm), _ptr(s), len(s), _ptr(sn), _ptr(t), len(t), _ptr(tn), _ptr(T0), _ptr(T),
             ctypes.byref(st))
    return _stats_dict(T, st)


def color_gradients(points, normals, colors, radius, max_nn=30, ctx=None):
    """r3d_color_gradients: the coloured registration's set-up on its own (InitializePointCloudForColoredICP).  Returns
    (intensity [n] = (r + g + b) / 3, gradient [n,3]): the least-squares gradient of the intensity in every point's tangent plane
    over its hybrid neighbourhood (radius, max_nn); zero with fewer than 4 neighbours or a singular system."""
    ctx = ctx or _lib.default_context()
    p, n, c = _c(points), _c(normals), _c(colors)
    inten, grad = np.empty(len(p)), np.empty((len(p), 3))
    if len(p) == 0:
        return inten, grad
    ctx.call("r3d_color_gradients", _ptr(p), _ptr(n), _ptr(c), len(p), float(radius), int(max_nn), _ptr(inten), _ptr(grad))
    return inten, grad


def _feat_rows(f):
    """a (33, N) feature array (o3d's Feature.data) as the C ABI's [N][33] rows"""
    f = np.asarray(f, dtype=np.float64)
    if f.ndim != 2 or f.shape[0] != FPFH_DIM:
        raise _lib.R3DError(-4, f"features must be a ({FPFH_DIM}, N) array, got {f.shape}")
    return np.ascontiguousarray(f.T)


def compute_fpfh_feature(points, normals, radius, max_nn=100, want_spfh=False, ctx=None):
    """o3d.pipelines.registration.compute_fpfh_feature(pcd, KDTreeSearchParamHybrid(radius, max_nn)).data: a (33, N) float64
    array (radius None or <= 0: KDTreeSearchParamKNN(max_nn)).  want_spfh=True returns (fpfh, spfh), the first stage's simplified
    histograms in the same shape.  Normals are required, as in Open3D."""
    ctx = ctx or _lib.default_context()
    p, n = _c(points), _c(normals)
    if n is None or len(n) != len(p):
        raise _lib.R3DError(-1, "compute_fpfh_feature: the cloud needs one normal per point")
    f = np.empty((len(p), FPFH_DIM))
    s = np.empty((len(p), FPFH_DIM)) if want_spfh else None
    if len(p):
        ctx.call("r3d_compute_fpfh", _ptr(p), _ptr(n), len(p), float(radius) if radius else -1.0, int(max_nn), _ptr(f), _ptr(s))
    return (f.T, s.T) if want_spfh else f.T


def fpfh_from_spfh(points, spfh, radius, max_nn=100, ctx=None):
    """r3d_fpfh_from_spfh: the second FPFH stage alone on a given (33, N) SPFH; returns the (33, N) FPFH"""
    ctx = ctx or _lib.default_context()
    p, s = _c(points), _feat_rows(spfh)
    if len(s) != len(p):
        raise _lib.R3DError(-1, "fpfh_from_spfh: one SPFH column per point")
    f = np.empty((len(p), FPFH_DIM))
    if len(p):
        ctx.call("r3d_fpfh_from_spfh", _ptr(p), len(p), float(radius) if radius else -1.0, int(max_nn), _ptr(s), _ptr(f))
    return f.T


def match_features(source_features, target_features, want_d2=True, ctx=None):
    """r3d_match_features: (nn [ns] int32, d2 [ns]) -- for every source column the target column at the smallest squared
    distance (float64, summed in row order), the smaller index on ties.  Features are (33, N) arrays."""
    ctx = ctx or _lib.default_context()
    s, t = _feat_rows(source_features), _feat_rows(target_features)
    nn = np.empty(len(s), np.int32)
    d2 = np.empty(len(s)) if want_d2 else None
    if len(s):
        ctx.call("r3d_match_features", _ptr(s), len(s), _ptr(t), len(t), FPFH_DIM, nn.ctypes.data_as(_vp), _ptr(d2))
    return nn, d2


def correspondences_from_features(source_features, target_features, mutual_filter=False, mutual_consistent_ratio=0.1, ctx=None):
    """o3d.pipelines.registration.correspondences_from_features: int32 [M, 2] rows (source index, target index), one per source
    feature.  mutual_filter keeps (i, j) only if i is also j's nearest source feature; if fewer than
    mutual_consistent_ratio * ns pairs survive, the unfiltered list is returned (Open3D's fall-back).  The two searches run on
    the device, the filter here."""
    nn_st, _ = match_features(source_features, target_features, False, ctx)
    ns = len(nn_st)
    corres = np.stack([np.arange(ns, dtype=np.int32), nn_st], 1)
    if not mutual_filter or ns == 0:
        return corres
    nn_ts, _ = match_features(target_features, source_features, False, ctx)
    mutual = corres[nn_ts[nn_st] == np.arange(ns)]
    return corres if len(mutual) < mutual_consistent_ratio * ns else mutual


def _ransac_params(max_correspondence_distance, ransac_n, edge_length, checker_distance, max_iteration, confidence, seed, batch):
    """edge_length None: no edge-length checker; checker_distance None: max_correspondence_distance (the scripts' usage), 0: none"""
    cd = max_correspondence_distance if checker_distance is None else checker_distance
    return RansacParams(float(max_correspondence_distance), float(edge_length or 0.0), float(cd or 0.0), float(confidence),
                        int(max_iteration), int(seed) & 0xFFFFFFFFFFFFFFFF, int(ransac_n), int(batch))


def _corres_rows(corres):
    c = np.ascontiguousarray(corres, dtype=np.int32)
    if c.ndim != 2 or c.shape[1] != 2:
        raise _lib.R3DError(-1, f"correspondences must be an [M, 2] array, got {c.shape}")
    return c


def _ransac_dict(T, st, **extra):
    return dict(T=T, fitness=st.fitness, inlier_rmse=st.inlier_rmse, iterations=st.iterations, validated=st.validated,
                best_hypothesis=st.best_hypothesis, inliers=st.inliers, setup_ms=st.setup_ms, loop_ms=st.loop_ms, **extra)


def registration_ransac_based_on_correspondence(source, target, corres, max_correspondence_distance, ransac_n=3, edge_length=0.9,
                                                checker_distance=None, max_iteration=100000, confidence=0.999, seed=0, batch=0, ctx=None):
    """o3d.pipelines.registration.registration_ransac_based_on_correspondence with TransformationEstimationPointToPoint(False),
    CorrespondenceCheckerBasedOnEdgeLength(edge_length), CorrespondenceCheckerBasedOnDistance(checker_distance) and
    RANSACConvergenceCriteria(max_iteration, confidence), as a pure function of (inputs, seed): DESIGN.md section 4 ("RANSAC").
    edge_length None: no edge checker.  checker_distance None: max_correspondence_distance; 0: no distance checker.
    Returns dict(T, fitness, inlier_rmse, correspondence_set [K, 2] int32, iterations, validated, best_hypothesis, inliers,
    setup_ms, loop_ms); nothing survived: T = identity, fitness 0, best_hypothesis -1."""
    ctx = ctx or _lib.default_context()
    s, t, c = _c(source), _c(target), _corres_rows(corres)
    prm = _ransac_params(max_correspondence_distance, ransac_n, edge_length, checker_distance, max_iteration, confidence, seed, batch)
    T, st = np.empty((4, 4)), RansacStats()
    mask = np.zeros(len(c), np.uint8)
    ctx.call("r3d_ransac_correspondence", ctypes.byref(prm), _ptr(s), len(s), _ptr(t), len(t), c.ctypes.data_as(_vp), len(c), _ptr(T),
             mask.ctypes.data_as(_vp), ctypes.byref(st))
    return _ransac_dict(T, st, correspondence_set=c[mask != 0])


def registration_ransac_based_on_feature_matching(source, target, source_features, target_features, mutual_filter,
                                                  max_correspondence_distance, ransac_n=3, edge_length=0.9, checker_distance=None,
                                                  max_iteration=100000, confidence=0.999, seed=0, batch=0, mutual_consistent_ratio=0.1,
                                                  ctx=None):
    """o3d's function of that name: correspondences_from_features(source_features, target_features, mutual_filter,
    mutual_consistent_ratio) followed by registration_ransac_based_on_correspondence.  Features are (33, N) arrays."""
    corres = correspondences_from_features(source_features, target_features, mutual_filter, mutual_consistent_ratio, ctx)
    return registration_ransac_based_on_correspondence(source, target, corres, max_correspondence_distance, ransac_n, edge_length,
                                                       checker_distance, max_iteration, confidence, seed, batch, ctx)


def debug_ransac_hypotheses(source, target, corres, h0, count, max_correspondence_distance, ransac_n=3, edge_length=0.9,
                            checker_distance=None, seed=0, ctx=None):
    """r3d_debug_ransac_hypotheses: hypotheses h0 .. h0 + count - 1 without the best / stop rule: dict(samples [count, 4] int32
    (-1 where unused), flags (bit 0 edge checker passed, bit 1 distance checker passed), T [count, 3, 4] (zeros where bit 0 is 0),
    inliers, err2 (0 unless both bits are set))."""
    ctx = ctx or _lib.default_context()
    s, t, c = _c(source), _c(target), _corres_rows(corres)
    prm = _ransac_params(max_correspondence_distance, ransac_n, edge_length, checker_distance, 1, 0.999, seed, 0)
    n = max(int(count), 0)
    samples, flags, inl = np.empty((n, 4), np.int32), np.empty(n, np.int32), np.empty(n, np.int32)
    T, err2 = np.empty((n, 3, 4)), np.empty(n)
    ctx.call("r3d_debug_ransac_hypotheses", ctypes.byref(prm), _ptr(s), len(s), _ptr(t), len(t), c.ctypes.data_as(_vp), len(c), int(h0),
             int(count), samples.ctypes.data_as(_vp), flags.ctypes.data_as(_vp), _ptr(T), inl.ctypes.data_as(_vp), _ptr(err2))
    return dict(samples=samples, flags=flags, T=T, inliers=inl, err2=err2)


def _fgr_params(division_factor=1.4, use_absolute_scale=False, decrease_mu=True, maximum_correspondence_distance=0.025, iteration_number=64,
                tuple_scale=0.95, maximum_tuple_count=1000, tuple_test=True, seed=0, batch=0):
    """o3d.pipelines.registration.FastGlobalRegistrationOption's names and defaults, plus seed and batch"""
    return FgrParams(float(division_factor), float(maximum_correspondence_distance), float(tuple_scale), int(seed) & 0xFFFFFFFFFFFFFFFF,
                     int(iteration_number), int(maximum_tuple_count), int(bool(use_absolute_scale)), int(bool(decrease_mu)),
                     int(bool(tuple_test)), int(batch))


def _fgr_dict(T, st, **extra):
    return dict(T=T, fitness=st.fitness, inlier_rmse=st.inlier_rmse, correspondences=st.correspondences, matched=st.matched,
                trials=st.trials, tuples=st.tuples, pairs=st.pairs, scale_global=st.scale_global, scale_start=st.scale_start,
                final_par=st.final_par, setup_ms=st.setup_ms, loop_ms=st.loop_ms, **extra)


def _evaluation_set(s, t, T, max_distance, ctx):
    """the correspondence set of the registration loop's evaluation at pose T: (source index, nearest target index) rows"""
    corr, _ = debug_icp_correspondences(s, t, max_distance, T, False, ctx)
    hit = np.nonzero(corr >= 0)[0]
    return np.stack([hit.astype(np.int32), corr[hit]], 1)


def registration_fgr_based_on_correspondence(source, target, corres, ctx=None, **option):
    """o3d.pipelines.registration.registration_fgr_based_on_correspondence(source, target, corres, FastGlobalRegistrationOption(
    **option)) as a pure function of (inputs, option, seed): DESIGN.md section 4 ("FGR").  `option`: division_factor,
    use_absolute_scale, decrease_mu, maximum_correspondence_distance, iteration_number, tuple_scale, maximum_tuple_count,
    tuple_test (Open3D's names and defaults), seed (the tuple sampler's) and batch (trials per launch; never changes the result).
    Returns dict(T, fitness, inlier_rmse, correspondence_set [K, 2] int32, correspondences, matched, trials, tuples, pairs,
    scale_global, scale_start, final_par, setup_ms, loop_ms); fitness, inlier_rmse and the set are the registration loop's
    evaluation at T with maximum_correspondence_distance.  Fewer than 10 rows: T is the centroid-to-centroid translation."""
    ctx = ctx or _lib.default_context()
    s, t, c = _c(source), _c(target), _corres_rows(corres)
    prm = _fgr_params(**option)
    T, st = np.empty((4, 4)), FgrStats()
    ctx.call("r3d_fgr_correspondence", ctypes.byref(prm), _ptr(s), len(s), _ptr(t), len(t), c.ctypes.data_as(_vp), len(c), _ptr(T),
             ctypes.byref(st))
    return _fgr_dict(T, st, correspondence_set=_evaluation_set(s, t, T, prm.maximum_correspondence_distance, ctx))


def registration_fgr_based_on_feature_matching(source, target, source_features, target_features, ctx=None, **option):
    """o3d's function of that name: the mutual pairs of the two nearest-feature searches (the plain cross-check, in ascending
    source index; not correspondences_from_features' mutual_consistent_ratio fall-back), then the tuple test and the loop of
    registration_fgr_based_on_correspondence, all on the device.  Features are (33, N) arrays."""
    ctx = ctx or _lib.default_context()
    s, t, sf, tf = _c(source), _c(target), _feat_rows(source_features), _feat_rows(target_features)
    if len(sf) != len(s) or len(tf) != len(t):
        raise _lib.R3DError(-1, "registration_fgr_based_on_feature_matching: one feature column per point")
    prm = _fgr_params(**option)
    T, st = np.empty((4, 4)), FgrStats()
    ctx.call("r3d_fgr_feature_matching", ctypes.byref(prm), _ptr(s), len(s), _ptr(t), len(t), _ptr(sf), _ptr(tf), FPFH_DIM, _ptr(T),
             ctypes.byref(st))
    return _fgr_dict(T, st, correspondence_set=_evaluation_set(s, t, T, prm.maximum_correspondence_distance, ctx))


def debug_fgr_tuples(source, target, corres, t0, count, ctx=None, **option):
    """r3d_debug_fgr_tuples: trials t0 .. t0 + count - 1 of the tuple test over the normalised pairs, without the cut:
    dict(samples [count, 3] int32, flags [count] int32)"""
    ctx = ctx or _lib.default_context()
    s, t, c = _c(source), _c(target), _corres_rows(corres)
    prm = _fgr_params(**option)
    n = max(int(count), 0)
    samples, flags = np.empty((n, 3), np.int32), np.empty(n, np.int32)
    ctx.call("r3d_debug_fgr_tuples", ctypes.byref(prm), _ptr(s), len(s), _ptr(t), len(t), c.ctypes.data_as(_vp), len(c), int(t0), int(count),
             samples.ctypes.data_as(_vp), flags.ctypes.data_as(_vp))
    return dict(samples=samples, flags=flags)


def debug_fgr_optimize(source, target, pairs, ctx=None, **option):
    """r3d_debug_fgr_optimize: the loop alone on the given pairs: dict(trace_T [iteration_number, 4, 4], trace_par
    [iteration_number]), the composed transform (target -> source) and the annealing parameter after every iteration, in
    normalised units; fewer than 10 pairs: the start state"""
    ctx = ctx or _lib.default_context()
    s, t, c = _c(source), _c(target), _corres_rows(pairs)
    prm = _fgr_params(**option)
    it = max(prm.iteration_number, 0)
    trace_T, trace_par = np.empty((it, 4, 4)), np.empty(it)
    ctx.call("r3d_debug_fgr_optimize", ctypes.byref(prm), _ptr(s), len(s), _ptr(t), len(t), c.ctypes.data_as(_vp), len(c), _ptr(trace_T),
             _ptr(trace_par))
    return dict(trace_T=trace_T, trace_par=trace_par)


def _colored_params(max_correspondence_distance, lambda_geometric, max_iteration, relative_fitness, relative_rmse, gradient_radius,
                    gradient_max_nn):
    return _lib.ColoredIcpParams(_lib.IcpParams(COLORED, int(max_iteration), float(max_correspondence_distance), float(relative_fitness),
                                                float(relative_rmse), 0.0),
                                 float(lambda_geometric), float(gradient_radius) if gradient_radius else -1.0, int(gradient_max_nn), 0)


def registration_colored(source, source_colors, target, target_normals, target_colors, max_correspondence_distance, init=None,
                         lambda_geometric=0.968, max_iteration=30, relative_fitness=1e-6, relative_rmse=1e-6, gradient_radius=None,
                         gradient_max_nn=30, ctx=None):
    """registration_colored_icp (r3d_icp_colored): point-to-plane with a photometric residual per correspondence, weighted
    lambda_geometric : 1 - lambda_geometric.  Colours are [n,3] in [0,1]; gradient_radius None: 2 * max_correspondence_distance.
    Returns the same dict as registration()."""
    ctx = ctx or _lib.default_context()
    s, sc, t, tn, tc = _c(source), _c(source_colors), _c(target), _c(target_normals), _c(target_colors)
    T0 = None if init is None else np.ascontiguousarray(init, dtype=np.float64).reshape(4, 4)
    T = np.empty((4, 4))
    prm = _colored_params(max_correspondence_distance, lambda_geometric, max_iteration, relative_fitness, relative_rmse, gradient_radius,
                          gradient_max_nn)
    st = _lib.IcpStats()
    ctx.call("r3d_icp_colored", ctypes.byref(prm), _ptr(s), _ptr(sc), len(s), _ptr(t), _ptr(tn), _ptr(tc), len(t), _ptr(T0), _ptr(T),
             ctypes.byref(st))
    return _stats_dict(T, st)


def debug_icp_sums_colored(source, source_colors, target, target_normals, target_colors, max_distance, T=None, lambda_geometric=0.968,
                           gradient_radius=0.0, gradient_max_nn=0, ctx=None):
    """r3d_debug_icp_sums_colored: (sums [29], records [nt,4]) of one evaluation of the coloured registration loop at pose T, as
    the device reduces them for its step, and the target's (intensity, gradient) records as the set-up computed them, in the
    caller's numbering.  gradient_radius 0: 2 * max_distance; gradient_max_nn 0: 30.  The slots' meaning: include/r3d.h."""
    ctx = ctx or _lib.default_context()
    s, sc, t, tn, tc = _c(source), _c(source_colors), _c(target), _c(target_normals), _c(target_colors)
    T0 = None if T is None else np.ascontiguousarray(T, dtype=np.float64).reshape(4, 4)
    prm = _colored_params(max_distance, lambda_geometric, 0, 0.0, 0.0, gradient_radius, gradient_max_nn)
    sums, records = np.empty(29), np.empty((len(t), 4))
    ctx.call("r3d_debug_icp_sums_colored", ctypes.byref(prm), _ptr(s), _ptr(sc), len(s), _ptr(t), _ptr(tn), _ptr(tc), len(t), _ptr(T0),
             _ptr(sums), _ptr(records))
    return sums, records


def align_point_clouds(source, target, threshold=0.02, voxel_size=0.01, max_iteration=100, mode=P2P, normal_radius=None,
                       normal_max_nn=30, source_colors=None, init=None, relative_fitness=1e-6, relative_rmse=1e-6,
                       gicp_epsilon=1e-3, ctx=None):
    """The body of PointCloudAlignment.align_point_clouds (pointcloud_alignment.py:6-43) as one device-resident call
    (r3d_align_point_clouds): voxel_down_sample both -> normals on both -> registration -> transform the source.
    Returns dict(points, colors, normals, T, fitness, ...): the down-sampled, transformed source."""
    ctx = ctx or _lib.default_context()
    s, t, sc = _c(source), _c(target), _c(source_colors)
    T0 = None if init is None else np.ascontiguousarray(init, dtype=np.float64).reshape(4, 4)
    prm = AlignParams(_lib.IcpParams(int(mode), int(max_iteration), float(threshold), float(relative_fitness),
                                     float(relative_rmse), float(gicp_epsilon)),
                      float(voxel_size) if voxel_size else -1.0,
                      float(normal_radius) if normal_radius else (2.0 * voxel_size if voxel_size else -1.0),
                      int(normal_max_nn) if normal_max_nn else 0, 0)
    op = np.empty((len(s), 3))
    oc = np.empty((len(s), 3)) if sc is not None else None
    on = np.empty((len(s), 3)) if prm.normal_max_nn > 0 else None
    T = np.empty((4, 4))
    m = ctypes.c_int64()
    st = _lib.IcpStats()
    ctx.call("r3d_align_point_clouds", ctypes.byref(prm), _ptr(s), _ptr(sc), len(s), _ptr(t), len(t), _ptr(T0), _ptr(op),
             _ptr(oc), _ptr(on), ctypes.byref(m), _ptr(T), ctypes.byref(st))
    m = m.value
    return dict(points=op[:m].copy(), colors=None if oc is None else oc[:m].copy(), normals=None if on is None else on[:m].copy(),
                T=T, fitness=st.fitness, inlier_rmse=st.inlier_rmse, iterations=st.iterations, converged=bool(st.converged),
                correspondences=st.correspondences, setup_ms=st.setup_ms, loop_ms=st.loop_ms)


def _stats_dict(T, st):
    return dict(T=T, fitness=st.fitness, inlier_rmse=st.inlier_rmse, iterations=st.iterations, converged=bool(st.converged),
                correspondences=st.correspondences, setup_ms=st.setup_ms, loop_ms=st.loop_ms)


class ResidentModel:
    """The growing `combined_pcd` of the scanning loops (main.py:28,34-54; test/GICP1.py:134-155) kept in HBM (r3d_model_*):
    per frame only the frame is uploaded and the 4x4 + statistics come back; download() fetches the model once at the end."""

    def __init__(self, ctx=None):
        self.ctx = ctx or _lib.default_context()
        h = _vp()
        self.ctx.check(self.ctx._lib.r3d_model_create(self.ctx._h, ctypes.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None) and getattr(self.ctx, "_h", None):
            self.ctx._lib.r3d_model_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    def _call(self, name, *args):
        self.ctx.check(getattr(self.ctx._lib, name)(self._h, *args))

    def size(self):
        n, hc, hn = ctypes.c_int64(), ctypes.c_int32(), ctypes.c_int32()
        self._call("r3d_model_size", ctypes.byref(n), ctypes.byref(hc), ctypes.byref(hn))
        return n.value, bool(hc.value), bool(hn.value)

    def __len__(self):
        return self.size()[0]

    def voxel_table_stats(self):
        """(voxels in the resident legacy voxel table, full rebuilds, incremental updates) -- r3d_model_voxel_table_stats."""
        v, r, u = ctypes.c_int64(), ctypes.c_int32(), ctypes.c_int32()
        self._call("r3d_model_voxel_table_stats", ctypes.byref(v), ctypes.byref(r), ctypes.byref(u))
        return v.value, r.value, u.value

    def debug_voxel_table(self, voxel, cap=None):
        """r3d_model_debug_voxel_table: the model's legacy voxel grid as the next align_append(voxel_size=voxel) would see it,
        entry by entry in ascending (kx, ky, kz) order: keys (uint64, kx << 42 | ky << 21 | kz), sums [n,3], counts, means [n,3],
        box [6] and resident.  Without a resident table keys / sums / counts are None; with more than `cap` voxels (default: room
        for any table) every array is None and only n and resident are reported."""
        cap = self.size()[0] if cap is None else int(cap)
        keys, sums, counts = np.empty(cap, np.uint64), np.empty((cap, 3)), np.empty(cap, np.int32)
        means, box = np.empty((cap, 3)), np.empty(6)
        n, res = ctypes.c_int64(), ctypes.c_int32()
        self._call("r3d_model_debug_voxel_table", float(voxel), cap, _ptr(keys), _ptr(sums), _ptr(counts), _ptr(means), _ptr(box),
                   ctypes.byref(n), ctypes.byref(res))
        n, res = n.value, bool(res.value)
        if n > cap:
            return dict(n=n, resident=res, keys=None, sums=None, counts=None, means=None, box=None)
        tab = (keys[:n].copy(), sums[:n].copy(), counts[:n].copy()) if res else (None, None, None)
        return dict(n=n, resident=res, keys=tab[0], sums=tab[1], counts=tab[2], means=means[:n].copy(), box=box)

    def debug_fail_table_step(self, step):
        """r3d_model_debug_fail_table_step (test hook): the next voxel-table call returns an error when it reaches point `step` (1: a
        rebuild after its build kernel, 2: an update after the slice is added, 3: an update after its merge); one shot, 0 disarms."""
        self._call("r3d_model_debug_fail_table_step", int(step))

    def clear(self):
        self._call("r3d_model_clear")

    def append(self, points, colors=None, normals=None):
        p, c, n = _c(points), _c(colors), _c(normals)
        self._call("r3d_model_append", _ptr(p), _ptr(c), _ptr(n), len(p))

    def align_append(self, source, threshold=0.02, voxel_size=0.01, max_iteration=100, mode=P2P, normal_radius=None,
                     normal_max_nn=30, source_colors=None, relative_fitness=1e-6, relative_rmse=1e-6, gicp_epsilon=1e-3):
        """align_point_clouds(frame, model, threshold, voxel_size, max_iter) followed by model += aligned (main.py:48-49)."""
        s, sc = _c(source), _c(source_colors)
        prm = AlignParams(_lib.IcpParams(int(mode), int(max_iteration), float(threshold), float(relative_fitness),
                                         float(relative_rmse), float(gicp_epsilon)),
                          float(voxel_size) if voxel_size else -1.0,
                          float(normal_radius) if normal_radius else (2.0 * voxel_size if voxel_size else -1.0),
                          int(normal_max_nn) if normal_max_nn else 0, 0)
        T = np.empty((4, 4))
        st = _lib.IcpStats()
        m = ctypes.c_int64()
        self._call("r3d_model_align_append", ctypes.byref(prm), _ptr(s), _ptr(sc), len(s), _ptr(T), ctypes.byref(st), ctypes.byref(m))
        return dict(_stats_dict(T, st), appended=m.value)

    def register_append(self, source, threshold=0.02, mode=GICP, max_iteration=30, source_colors=None, source_normals=None,
                        relative_fitness=1e-6, relative_rmse=1e-6, gicp_epsilon=1e-3):
        """registration of the frame against the whole model, then model += transformed frame (test/GICP1.py:145-146)."""
        s, sc, sn = _c(source), _c(source_colors), _c(source_normals)
        prm = _lib.IcpParams(int(mode), int(max_iteration), float(threshold), float(relative_fitness), float(relative_rmse),
                             float(gicp_epsilon))
        T = np.empty((4, 4))
        st = _lib.IcpStats()
        self._call("r3d_model_register_append", ctypes.byref(prm), _ptr(s), _ptr(sc), _ptr(sn), len(s), _ptr(T), ctypes.byref(st))
        return _stats_dict(T, st)

    def append_depth(self, depth, camera, color=None):
        """First frame given as a depth image (uint16 [H,W]; color uint8 [H,W,3] optional): back-projected on the device."""
        d, c = _depth_args(depth, color)
        m = ctypes.c_int64()
        self._call("r3d_model_append_depth", d.ctypes.data_as(_vp), d.shape[1], d.shape[0], d.shape[1], ctypes.byref(camera),
                   c.ctypes.data_as(_vp) if c is not None else None, 3 * d.shape[1] if c is not None else 0, ctypes.byref(m))
        return m.value

    def align_append_depth(self, depth, camera, color=None, threshold=0.02, voxel_size=0.01, max_iteration=100, mode=P2P,
                           normal_radius=None, normal_max_nn=30, relative_fitness=1e-6, relative_rmse=1e-6, gicp_epsilon=1e-3):
        """main.py:48-49 for a frame that is still a depth image: create_from_rgbd_image + flip on the device, then align_append."""
        d, c = _depth_args(depth, color)
        prm = AlignParams(_lib.IcpParams(int(mode), int(max_iteration), float(threshold), float(relative_fitness),
                                         float(relative_rmse), float(gicp_epsilon)),
                          float(voxel_size) if voxel_size else -1.0,
                          float(normal_radius) if normal_radius else (2.0 * voxel_size if voxel_size else -1.0),
                          int(normal_max_nn) if normal_max_nn else 0, 0)
        T = np.empty((4, 4))
        st = _lib.IcpStats()
        npts, m = ctypes.c_int64(), ctypes.c_int64()
        self._call("r3d_model_align_append_depth", ctypes.byref(prm), d.ctypes.data_as(_vp), d.shape[1], d.shape[0], d.shape[1],
                   ctypes.byref(camera), c.ctypes.data_as(_vp) if c is not None else None, 3 * d.shape[1] if c is not None else 0,
                   _ptr(T), ctypes.byref(st), ctypes.byref(npts), ctypes.byref(m))
        return dict(_stats_dict(T, st), frame_points=npts.value, appended=m.value)

    def estimate_normals(self, radius=0.05, max_nn=30):
        self._call("r3d_model_estimate_normals", float(radius) if radius else -1.0, int(max_nn))

    def download(self):
        n, hc, hn = self.size()
        p = np.empty((n, 3))
        c = np.empty((n, 3)) if hc else None
        nr = np.empty((n, 3)) if hn else None
        if n:
            self._call("r3d_model_download", _ptr(p), _ptr(c), _ptr(nr))
        return p, c, nr


def disparity_to_cloud_resident(d_disp, width, height, Q, d_out_points, d_out_normals, capacity, min_disparity=0, max_depth=None,
                                pose=None, voxel=0.01, normal_radius=None, max_nn=30, ctx=None, d_color=None, color_stride=None,
                                color_channels=3, color_order="bgr", d_out_colors=None):
    """r3d_disparity_to_cloud_resident: like disparity_to_cloud_device, but the cloud is written to the caller's DEVICE buffers
    (pointers as ints, `capacity` triplets each; e.g. torch tensors' data_ptr()).  Returns the number of points.
    d_color / color_stride / color_channels / color_order as in disparity_to_cloud_device; the colours go to d_out_colors
    (r3d_disparity_to_cloud_color_resident)."""
    ctx = ctx or _lib.default_context()
    Q = np.ascontiguousarray(Q, dtype=np.float64).reshape(4, 4)
    P = None if pose is None else np.ascontiguousarray(pose, dtype=np.float64).reshape(4, 4)
    m = ctypes.c_int64()
    head = (_vp(d_disp), int(width), int(height), _ptr(Q), int(min_disparity) * 16, float(max_depth) if max_depth else -1.0, _ptr(P),
            float(voxel) if voxel else -1.0, float(normal_radius) if normal_radius else -1.0, int(max_nn) if max_nn else 0)
    d_nrm = _vp(d_out_normals) if d_out_normals else None
    if d_color is None:
        if d_out_colors:
            raise ValueError("d_out_colors given without d_color")
        ctx.call("r3d_disparity_to_cloud_resident", *head, int(capacity), _vp(d_out_points), d_nrm, ctypes.byref(m))
    else:
        ctx.call("r3d_disparity_to_cloud_color_resident", *head, *_color_args(d_color, width, color_stride, color_channels, color_order),
                 int(capacity), _vp(d_out_points), d_nrm, _vp(d_out_colors) if d_out_colors else None, ctypes.byref(m))
    return m.value


def registration_device(d_source, ns, d_target, nt, max_correspondence_distance, init=None, mode=P2P, max_iteration=30,
                        relative_fitness=1e-6, relative_rmse=1e-6, d_source_normals=None, d_target_normals=None, gicp_epsilon=1e-3,
                        ctx=None):
    """r3d_icp_dev: registration of two clouds that are already in HBM (device pointers as ints)."""
    ctx = ctx or _lib.default_context()
    T0 = None if init is None else np.ascontiguousarray(init, dtype=np.float64).reshape(4, 4)
    T = np.empty((4, 4))
    prm = _lib.IcpParams(int(mode), int(max_iteration), float(max_correspondence_distance), float(relative_fitness),
                         float(relative_rmse), float(gicp_epsilon))
    st = _lib.IcpStats()
    ctx.call("r3d_icp_dev", ctypes.byref(prm), _vp(d_source), int(ns), _vp(d_source_normals) if d_source_normals else None,
             _vp(d_target), int(nt), _vp(d_target_normals) if d_target_normals else None, _ptr(T0), _ptr(T), ctypes.byref(st))
    return _stats_dict(T, st)


def registration_colored_device(d_source, d_source_colors, ns, d_target, d_target_normals, d_target_colors, nt,
                                max_correspondence_distance, init=None, lambda_geometric=0.968, max_iteration=30, relative_fitness=1e-6,
                                relative_rmse=1e-6, gradient_radius=None, gradient_max_nn=30, ctx=None):
    """r3d_icp_colored_dev: registration_colored on clouds that are already in HBM (device pointers as ints)."""
    ctx = ctx or _lib.default_context()
    T0 = None if init is None else np.ascontiguousarray(init, dtype=np.float64).reshape(4, 4)
    T = np.empty((4, 4))
    prm = _colored_params(max_correspondence_distance, lambda_geometric, max_iteration, relative_fitness, relative_rmse, gradient_radius,
                          gradient_max_nn)
    st = _lib.IcpStats()
    ctx.call("r3d_icp_colored_dev", ctypes.byref(prm), _vp(d_source), _vp(d_source_colors) if d_source_colors else None, int(ns),
             _vp(d_target), _vp(d_target_normals) if d_target_normals else None, _vp(d_target_colors) if d_target_colors else None,
             int(nt), _ptr(T0), _ptr(T), ctypes.byref(st))
    return _stats_dict(T, st)


def compute_fpfh_feature_device(d_points, d_normals, n, radius, d_fpfh, max_nn=100, d_spfh=None, ctx=None):
    """r3d_compute_fpfh_dev: FPFH of a cloud that is already in HBM into d_fpfh ([n][33] float64 rows, a device pointer as int;
    d_spfh optionally receives the first stage).  Enqueued on the context stream: ctx.sync() before reading the result."""
    ctx = ctx or _lib.default_context()
    ctx.call("r3d_compute_fpfh_dev", _vp(d_points), _vp(d_normals) if d_normals else None, int(n), float(radius) if radius else -1.0,
             int(max_nn), _vp(d_fpfh), _vp(d_spfh) if d_spfh else None)


def match_features_device(d_source_features, ns, d_target_features, nt, d_nn, d_d2=None, ctx=None):
    """r3d_match_features_dev: match_features on [n][33] rows in HBM into d_nn (int32 [ns]) / d_d2 (float64 [ns]); enqueued only"""
    ctx = ctx or _lib.default_context()
    ctx.call("r3d_match_features_dev", _vp(d_source_features), int(ns), _vp(d_target_features), int(nt), FPFH_DIM, _vp(d_nn),
             _vp(d_d2) if d_d2 else None)


def debug_fpfh_stages(d_points, d_normals, n, radius, d_fpfh, max_nn=100, ctx=None):
    """r3d_debug_fpfh_stages: dict of device ms: k_knn_graph at the same (n, k, radius), and the two FPFH stages"""
    ctx = ctx or _lib.default_context()
    ms = (ctypes.c_float * 3)()
    ctx.call("r3d_debug_fpfh_stages", _vp(d_points), _vp(d_normals), int(n), float(radius) if radius else -1.0, int(max_nn), _vp(d_fpfh), ms)
    return dict(search_ms=ms[0], spfh_ms=ms[1], fpfh_ms=ms[2])


def registration_ransac_based_on_correspondence_device(d_source, ns, d_target, nt, d_corres, m, max_correspondence_distance, ransac_n=3,
                                                       edge_length=0.9, checker_distance=None, max_iteration=100000, confidence=0.999,
                                                       seed=0, batch=0, d_inlier_mask=None, ctx=None):
    """r3d_ransac_correspondence_dev: clouds ([n][3] float64) and pairs ([m][2] int32) already in HBM (device pointers as int).
    Returns when the loop has finished.  d_inlier_mask (optional, uint8 [m] on the device) receives the winner's mask; the dict
    has no correspondence_set."""
    ctx = ctx or _lib.default_context()
    prm = _ransac_params(max_correspondence_distance, ransac_n, edge_length, checker_distance, max_iteration, confidence, seed, batch)
    T, st = np.empty((4, 4)), RansacStats()
    ctx.call("r3d_ransac_correspondence_dev", ctypes.byref(prm), _vp(d_source), int(ns), _vp(d_target), int(nt), _vp(d_corres), int(m), _ptr(T),
             _vp(d_inlier_mask) if d_inlier_mask else None, ctypes.byref(st))
    return _ransac_dict(T, st)


def registration_ransac_based_on_feature_matching_device(d_source, ns, d_target, nt, d_source_features, d_target_features, mutual_filter,
                                                         max_correspondence_distance, mutual_consistent_ratio=0.1, ctx=None, **kw):
    """The feature-matching form on device arrays ([n][33] float64 feature rows): both searches through r3d_match_features_dev, the
    mutual filter on the host (two int32 [n] read-backs), the estimator through r3d_ransac_correspondence_dev.  Returns the dict of
    the device form plus correspondence_set."""
    ctx = ctx or _lib.default_context()
    d_nn = ctx.alloc(4 * max(ns, nt))
    try:
        nn_st, nn_ts = np.empty(ns, np.int32), np.empty(nt, np.int32)
        match_features_device(d_source_features, ns, d_target_features, nt, d_nn, None, ctx)
        ctx.d2h(nn_st, d_nn)
        corres = np.stack([np.arange(ns, dtype=np.int32), nn_st], 1)
        if mutual_filter and ns:
            match_features_device(d_target_features, nt, d_source_features, ns, d_nn, None, ctx)
            ctx.d2h(nn_ts, d_nn)
            mutual = corres[nn_ts[nn_st] == np.arange(ns)]
            corres = corres if len(mutual) < mutual_consistent_ratio * ns else mutual
    finally:
        ctx.free(d_nn)
    corres = np.ascontiguousarray(corres)
    d_c, d_m = ctx.to_device(corres), ctx.alloc(max(len(corres), 1))
    try:
        res = registration_ransac_based_on_correspondence_device(d_source, ns, d_target, nt, d_c, len(corres), max_correspondence_distance,
                                                                 d_inlier_mask=d_m, ctx=ctx, **kw)
        mask = np.empty(len(corres), np.uint8)
        ctx.d2h(mask, d_m)
    finally:
        ctx.free(d_c)
        ctx.free(d_m)
    res["correspondence_set"] = corres[mask != 0]
    return res


def registration_fgr_based_on_correspondence_device(d_source, ns, d_target, nt, d_corres, m, ctx=None, **option):
    """r3d_fgr_correspondence_dev: clouds ([n][3] float64) and pairs ([m][2] int32) already in HBM (device pointers as int).
    Returns when the result is ready; the dict of registration_fgr_based_on_correspondence without correspondence_set."""
    ctx = ctx or _lib.default_context()
    prm = _fgr_params(**option)
    T, st = np.empty((4, 4)), FgrStats()
    ctx.call("r3d_fgr_correspondence_dev", ctypes.byref(prm), _vp(d_source), int(ns), _vp(d_target), int(nt), _vp(d_corres), int(m), _ptr(T),
             ctypes.byref(st))
    return _fgr_dict(T, st)


def registration_fgr_based_on_feature_matching_device(d_source, ns, d_target, nt, d_source_features, d_target_features, ctx=None, **option):
    """r3d_fgr_feature_matching_dev: clouds and [n][33] float64 feature rows already in HBM; searches, cross-check, tuple test and
    loop without a host copy of any of them.  The dict of the host form without correspondence_set."""
    ctx = ctx or _lib.default_context()
    prm = _fgr_params(**option)
    T, st = np.empty((4, 4)), FgrStats()
    ctx.call("r3d_fgr_feature_matching_dev", ctypes.byref(prm), _vp(d_source), int(ns), _vp(d_target), int(nt), _vp(d_source_features),
             _vp(d_target_features), FPFH_DIM, _ptr(T), ctypes.byref(st))
    return _fgr_dict(T, st)


def transform_points_device(d_points, n, T, d_out, rotate_only=False, ctx=None):
    ctx = ctx or _lib.default_context()
    T = np.ascontiguousarray(T, dtype=np.float64).reshape(4, 4)
    ctx.call("r3d_transform_points_dev", _vp(d_points), int(n), _ptr(T), int(bool(rotate_only)), _vp(d_out))


def transform_blocks_device(blocks, ctx=None):
    """blocks: sequence of (d_in, n, T 4x4, d_out, rotate_only) -- every block moved by its own rigid transform in one launch per
    16 blocks (r3d_transform_blocks_dev); device pointers as ints, asynchronous on the context stream."""
    ctx = ctx or _lib.default_context()
    nb = len(blocks)
    if nb == 0:
        return
    pin = (ctypes.c_void_p * nb)(*[int(b[0]) for b in blocks])
    pout = (ctypes.c_void_p * nb)(*[int(b[3]) for b in blocks])
    cnt = np.ascontiguousarray([int(b[1]) for b in blocks], dtype=np.int64)
    Ts = np.ascontiguousarray(np.stack([np.asarray(b[2], dtype=np.float64).reshape(4, 4) for b in blocks]))
    ro = np.ascontiguousarray([1 if b[4] else 0 for b in blocks], dtype=np.int32)
    ctx.call("r3d_transform_blocks_dev", nb, ctypes.cast(pin, _vp), cnt.ctypes.data_as(_vp), _ptr(Ts), ro.ctypes.data_as(_vp), ctypes.cast(pout, _vp))


def backproject_depth(depth, camera, color=None, want_pixels=False, ctx=None):
    """create_from_rgbd_image(+ flip) of test/check84.py:155-159,172-178 (r3d_backproject_depth).  depth: uint16 [H,W];
    camera: depth_camera(...); color: uint8 [H,W,3] or None.  Returns (points [M,3], colors [M,3] or None[, pixel index [M]])."""
    ctx = ctx or _lib.default_context()
    d, c = _depth_args(depth, color)
    H, W = d.shape
    pts = np.empty((H * W, 3))
    col = np.empty((H * W, 3)) if c is not None else None
    pix = np.empty(H * W, np.int32) if want_pixels else None
    m = ctypes.c_int64()
    ctx.call("r3d_backproject_depth", d.ctypes.data_as(_vp), W, H, W, ctypes.byref(camera), c.ctypes.data_as(_vp) if c is not None else None,
             3 * W if c is not None else 0, _ptr(pts), _ptr(col), pix.ctypes.data_as(_vp) if want_pixels else None, ctypes.byref(m))
    n = m.value
    out = (pts[:n].copy(), col[:n].copy() if col is not None else None)
    return out + (pix[:n].copy(),) if want_pixels else out


# ---- RGB-D odometry ("RGB-D odometry") ----------------------------------------------------------------------
ODOMETRY_HYBRID, ODOMETRY_COLOR = 0, 1
_JACOBIANS = {"hybrid": ODOMETRY_HYBRID, "color": ODOMETRY_COLOR, "colour": ODOMETRY_COLOR, ODOMETRY_HYBRID: ODOMETRY_HYBRID,
              ODOMETRY_COLOR: ODOMETRY_COLOR}


class OdometryParams(ctypes.Structure):
    """r3d_odometry_params: Open3D's OdometryOption + the Jacobian term."""
    _fields_ = [("depth_diff_max", ctypes.c_double), ("depth_min", ctypes.c_double), ("depth_max", ctypes.c_double),
                ("iterations", ctypes.c_int32 * 4), ("levels", ctypes.c_int32), ("jacobian", ctypes.c_int32)]


class OdometryStats(ctypes.Structure):
    _fields_ = [("success", ctypes.c_int32), ("failed_level", ctypes.c_int32), ("failed_iteration", ctypes.c_int32),
                ("reserved", ctypes.c_int32), ("correspondences_init", ctypes.c_int64), ("correspondences", ctypes.c_int64),
                ("r2", ctypes.c_double), ("setup_ms", ctypes.c_double), ("loop_ms", ctypes.c_double)]


_i32, _dbl = ctypes.c_int32, ctypes.c_double
_odo_f32_sig = ([_vp, ctypes.POINTER(OdometryParams), _vp, _vp, _vp, _vp, _i32, _i32, _i32, _dbl, _dbl, _dbl, _dbl, _vp, _vp, _vp,
                 ctypes.POINTER(OdometryStats), _vp], ctypes.c_int)
_lib.register({
    "r3d_rgbd_odometry": ([_vp, ctypes.POINTER(OdometryParams), _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32,
                           ctypes.POINTER(DepthCamera), _vp, _vp, _vp, ctypes.POINTER(OdometryStats), _vp], ctypes.c_int),
    "r3d_rgbd_odometry_f32": _odo_f32_sig,
    "r3d_rgbd_odometry_f32_dev": _odo_f32_sig,
    "r3d_debug_rgbd_convert": ([_vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, ctypes.POINTER(DepthCamera), _vp, _vp], ctypes.c_int),
    "r3d_debug_rgbd_prepare": ([_vp, ctypes.POINTER(OdometryParams), _vp, _vp, _vp, _vp, _i32, _i32, _i32, _dbl, _dbl, _dbl, _dbl, _vp,
                                _vp, _vp, _vp, _vp, _i32, _vp, _i64p, _vp], ctypes.c_int),
    "r3d_debug_rgbd_iteration": ([_vp, ctypes.POINTER(OdometryParams), _vp, _vp, _vp, _vp, _i32, _i32, _i32, _dbl, _dbl, _dbl, _dbl, _vp,
                                  _i32, _vp, _vp, _i64p, _vp, _vp, ctypes.POINTER(_i32)], ctypes.c_int),
})


def odometry_params(jacobian="hybrid", depth_diff_max=0.03, depth_min=0.0, depth_max=4.0, iteration_number_per_pyramid_level=(20, 10, 5),
                    levels=None):
    """OdometryOption's fields as keywords.  iteration_number_per_pyramid_level: coarsest level first, as in Open3D; its length
    is the number of pyramid levels unless `levels` says otherwise (missing counts are 0)."""
    its = [int(i) for i in iteration_number_per_pyramid_level]
    levels = len(its) if levels is None else int(levels)
    if len(its) > 4 or jacobian not in _JACOBIANS:
        raise ValueError("at most 4 pyramid levels; jacobian is 'hybrid' or 'color'")
    return OdometryParams(float(depth_diff_max), float(depth_min), float(depth_max), (ctypes.c_int32 * 4)(*(its + [0] * 4)[:4]), levels,
                          _JACOBIANS[jacobian])


class RGBDImage:
    """create_from_color_and_depth(color, depth, depth_scale, depth_trunc, convert_rgb_to_intensity=True): the raw images and how
    to read them.  color: uint8 [H,W,3] or [H,W]; depth: uint16 [H,W].  The conversion itself runs on the device."""

    def __init__(self, color, depth, depth_scale=1000.0, depth_trunc=3.0, bgr=False):
        self.depth = np.ascontiguousarray(depth, dtype=np.uint16)
        self.color = np.ascontiguousarray(color, dtype=np.uint8)
        if self.depth.ndim != 2 or self.color.shape[:2] != self.depth.shape or self.color.ndim not in (2, 3) or \
                (self.color.ndim == 3 and self.color.shape[2] not in (1, 3)):
            raise ValueError(f"colour image {self.color.shape} and depth image {self.depth.shape} do not make an RGB-D image")
        self.channels = 1 if self.color.ndim == 2 else self.color.shape[2]
        self.depth_scale, self.depth_trunc, self.bgr = float(depth_scale), float(depth_trunc), bool(bgr)

    def planes(self, ctx=None):
        """-> intensity, depth as float32 [H,W] (r3d_debug_rgbd_convert)"""
        ctx = ctx or _lib.default_context()
        H, W = self.depth.shape
        cam = DepthCamera(1.0, 1.0, 0.0, 0.0, self.depth_scale, self.depth_trunc, 0, 0)
        inten, z = np.empty((H, W), np.float32), np.empty((H, W), np.float32)
        ctx.call("r3d_debug_rgbd_convert", _ptr(self.depth), _ptr(self.color), W, H, W, W * self.channels, self.channels, int(self.bgr),
                 ctypes.byref(cam), _ptr(inten), _ptr(z))
        return inten, z


def rgbd_image(color, depth, depth_scale=1000.0, depth_trunc=3.0, bgr=False):
    return RGBDImage(color, depth, depth_scale, depth_trunc, bgr)


def _intrinsic4(intrinsic):
    if isinstance(intrinsic, DepthCamera):
        return intrinsic.fx, intrinsic.fy, intrinsic.ppx, intrinsic.ppy
    if isinstance(intrinsic, dict):
        return tuple(float(intrinsic[k]) for k in ("fx", "fy", "ppx", "ppy"))
    a = np.asarray(intrinsic, dtype=np.float64)
    if a.size == 4:
        return tuple(float(v) for v in a.reshape(4))
    K = a.reshape(3, 3)
    return float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])


def _f32_frames(source, target):
    planes = [np.ascontiguousarray(p, dtype=np.float32) for p in (source[0], source[1], target[0], target[1])]
    if planes[0].ndim != 2 or any(p.shape != planes[0].shape for p in planes):
        raise ValueError("the four planes (source intensity, source depth, target intensity, target depth) must be 2-D and of one size")
    return planes


def _odometry_result(T, info, st, trace):
    res = dict(success=bool(st.success), T=T, info=info, failed_level=st.failed_level, failed_iteration=st.failed_iteration,
               correspondences_init=st.correspondences_init, correspondences=st.correspondences, r2=st.r2, setup_ms=st.setup_ms,
               loop_ms=st.loop_ms)
    if trace is not None:
        res["trace"] = trace
    return res


def rgbd_odometry(source, target, intrinsic, odo_init=None, jacobian="hybrid", want_trace=False, ctx=None, **option):
    """compute_rgbd_odometry with its statistics as a dict (T maps source camera coordinates to target camera coordinates).
    source / target: two RGBDImage (r3d_rgbd_odometry: the raw images go up and are converted on the device; both must share
    depth_scale, depth_trunc and channel order) or two (intensity, depth) pairs of float32 planes (r3d_rgbd_odometry_f32).
    intrinsic: depth_camera(...), a dict with fx / fy / ppx / ppy, a 3x3 matrix or (fx, fy, cx, cy)."""
    ctx = ctx or _lib.default_context()
    prm = odometry_params(jacobian, **option)
    fx, fy, cx, cy = _intrinsic4(intrinsic)
    init = None if odo_init is None else np.ascontiguousarray(odo_init, dtype=np.float64).reshape(4, 4)
    T, info, st = np.empty((4, 4)), np.empty((6, 6)), OdometryStats()
    trace = np.zeros((sum(prm.iterations[:prm.levels]) if 1 <= prm.levels <= 4 else 0, 4, 4)) if want_trace else None
    if isinstance(source, RGBDImage) and isinstance(target, RGBDImage):
        if (source.depth_scale, source.depth_trunc, source.bgr, source.channels, source.depth.shape) != \
                (target.depth_scale, target.depth_trunc, target.bgr, target.channels, target.depth.shape):
            raise ValueError("source and target RGB-D images differ in size, depth_scale, depth_trunc or channel order")
        H, W = source.depth.shape
        cam = DepthCamera(fx, fy, cx, cy, source.depth_scale, source.depth_trunc, 0, 0)
        ctx.call("r3d_rgbd_odometry", ctypes.byref(prm), _ptr(source.depth), _ptr(source.color), _ptr(target.depth), _ptr(target.color), W, H,
                 W, W * source.channels, source.channels, int(source.bgr), ctypes.byref(cam), _ptr(init), _ptr(T), _ptr(info), ctypes.byref(st),
                 _ptr(trace))
    else:
        si, sd, ti, td = _f32_frames(source, target)
        H, W = si.shape
        ctx.call("r3d_rgbd_odometry_f32", ctypes.byref(prm), _ptr(si), _ptr(sd), _ptr(ti), _ptr(td), W, H, W, fx, fy, cx, cy, _ptr(init),
                 _ptr(T), _ptr(info), ctypes.byref(st), _ptr(trace))
    return _odometry_result(T, info, st, trace)


def rgbd_odometry_device(d_source, d_target, width, height, intrinsic, odo_init=None, jacobian="hybrid", want_trace=False, ctx=None, **option):
    """r3d_rgbd_odometry_f32_dev: d_source / d_target are (intensity, depth) pairs of device pointers (as int) to contiguous
    float32 [height][width] planes.  Returns when the result is ready."""
    ctx = ctx or _lib.default_context()
    prm = odometry_params(jacobian, **option)
    fx, fy, cx, cy = _intrinsic4(intrinsic)
    init = None if odo_init is None else np.ascontiguousarray(odo_init, dtype=np.float64).reshape(4, 4)
    T, info, st = np.empty((4, 4)), np.empty((6, 6)), OdometryStats()
    trace = np.zeros((sum(prm.iterations[:prm.levels]) if 1 <= prm.levels <= 4 else 0, 4, 4)) if want_trace else None
    ctx.call("r3d_rgbd_odometry_f32_dev", ctypes.byref(prm), _vp(d_source[0]), _vp(d_source[1]), _vp(d_target[0]), _vp(d_target[1]), int(width),
             int(height), int(width), fx, fy, cx, cy, _ptr(init), _ptr(T), _ptr(info), ctypes.byref(st), _ptr(trace))
    return _odometry_result(T, info, st, trace)


def compute_rgbd_odometry(source, target, intrinsic, odo_init=None, jacobian="hybrid", want_trace=False, ctx=None, **option):
    """o3d.pipelines.odometry.compute_rgbd_odometry(source, target, intrinsic, odo_init, jacobian, OdometryOption(**option))
    (test/check84.py:239-241).  -> (success, T, info) as Open3D does[, trace [sum of iterations][4][4]]."""
    res = rgbd_odometry(source, target, intrinsic, odo_init, jacobian, want_trace, ctx, **option)
    out = (res["success"], res["T"], res["info"])
    return out + (res["trace"],) if want_trace else out


def debug_rgbd_prepare(source, target, intrinsic, odo_init=None, grad_level=0, ctx=None, **option):
    """r3d_debug_rgbd_prepare on (intensity, depth) float32 pairs.  -> dict(source=[(I_l, D_l)], target=[(I_l, D_l)],
    gradients=(dI/dx, dI/dy, dD/dx, dD/dy) of grad_level, correspondences_init, scales=(s_src, s_tgt))"""
    ctx = ctx or _lib.default_context()
    prm = odometry_params(**option)
    fx, fy, cx, cy = _intrinsic4(intrinsic)
    init = None if odo_init is None else np.ascontiguousarray(odo_init, dtype=np.float64).reshape(4, 4)
    si, sd, ti, td = _f32_frames(source, target)
    H, W = si.shape
    shapes = [(H >> l, W >> l) for l in range(max(prm.levels, 1))]
    total = sum(a * b for a, b in shapes)
    pyr = [np.empty(total, np.float32) for _ in range(4)]
    gl = min(max(int(grad_level), 0), len(shapes) - 1)
    grad = np.empty(shapes[gl] + (4,), np.float32)
    n, sc = ctypes.c_int64(), np.zeros(2)
    ctx.call("r3d_debug_rgbd_prepare", ctypes.byref(prm), _ptr(si), _ptr(sd), _ptr(ti), _ptr(td), W, H, W, fx, fy, cx, cy, _ptr(init),
             _ptr(pyr[0]), _ptr(pyr[1]), _ptr(pyr[2]), _ptr(pyr[3]), int(grad_level), _ptr(grad), ctypes.byref(n), _ptr(sc))
    offs = np.cumsum([0] + [a * b for a, b in shapes])
    cut = lambda p: [p[offs[l]:offs[l + 1]].reshape(shapes[l]) for l in range(len(shapes))]
    return dict(source=list(zip(cut(pyr[0]), cut(pyr[1]))), target=list(zip(cut(pyr[2]), cut(pyr[3]))),
                gradients=tuple(np.ascontiguousarray(grad[..., k]) for k in range(4)), correspondences_init=n.value, scales=(sc[0], sc[1]))


def debug_rgbd_iteration(source, target, intrinsic, level, pose, odo_init=None, jacobian="hybrid", ctx=None, **option):
    """r3d_debug_rgbd_iteration.  -> dict(corr int32 [n][4] rows (u_s, v_s, u_t, v_t), sums [29], T pose after the step, ok)"""
    ctx = ctx or _lib.default_context()
    prm = odometry_params(jacobian, **option)
    fx, fy, cx, cy = _intrinsic4(intrinsic)
    init = None if odo_init is None else np.ascontiguousarray(odo_init, dtype=np.float64).reshape(4, 4)
    pose = np.ascontiguousarray(pose, dtype=np.float64).reshape(4, 4)
    si, sd, ti, td = _f32_frames(source, target)
    H, W = si.shape
    lv = min(max(int(level), 0), 3)
    corr = np.empty(((H >> lv) * (W >> lv), 4), np.int32)
    n, ok, sums, T = ctypes.c_int64(), _i32(), np.empty(29), np.empty((4, 4))
    ctx.call("r3d_debug_rgbd_iteration", ctypes.byref(prm), _ptr(si), _ptr(sd), _ptr(ti), _ptr(td), W, H, W, fx, fy, cx, cy, _ptr(init),
             int(level), _ptr(pose), _ptr(corr), ctypes.byref(n), _ptr(sums), _ptr(T), ctypes.byref(ok))
    return dict(corr=corr[:n.value].copy(), sums=sums, T=T, ok=bool(ok.value))
