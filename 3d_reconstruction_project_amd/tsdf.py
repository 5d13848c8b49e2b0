"""o3d.pipelines.integration.ScalableTSDFVolume on the device ("TSDF volume"; C ABI: r3d_tsdf_*).
test/check84.py:41-44,295,307: every posed RGB-D frame is integrated into a volume and a surface is extracted from it."""
import ctypes
import enum

import numpy as np

from . import _lib, cloud_ops
from .pointcloud import PointCloud, TriangleMesh

_vp, _i32, _i64, _dbl = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_double
_i64p = ctypes.POINTER(ctypes.c_int64)
UNIT_VOXELS = 16 ** 3


class TSDFVolumeColorType(enum.IntEnum):
    """open3d.pipelines.integration.TSDFVolumeColorType; Gray32 is refused (R3D_E_UNSUPPORTED)"""
    NoColor = 0
    RGB8 = 1
    Gray32 = 2


class TsdfParams(ctypes.Structure):
    _fields_ = [("voxel_length", _dbl), ("sdf_trunc", _dbl), ("color_type", _i32), ("volume_unit_resolution", _i32),
                ("depth_sampling_stride", _i32), ("initial_units", _i32)]


class TsdfInfo(ctypes.Structure):
    _fields_ = [("units", _i64), ("frames", _i64), ("touched", _i64), ("capacity", _i32), ("growths", _i32), ("touch_ms", _dbl),
                ("integrate_ms", _dbl)]


_integrate_f32_sig = ([_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _dbl, _dbl, _dbl, _dbl, _vp], ctypes.c_int)
_extract_sig = ([_vp, _vp, _i64, _vp, _vp, _vp, _i64p], ctypes.c_int)
_mesh_sig = ([_vp, _vp, _i64, _i64, _vp, _vp, _vp, _i64p, _i64p], ctypes.c_int)
_lib.register({
    "r3d_tsdf_create": ([_vp, ctypes.POINTER(TsdfParams), ctypes.POINTER(_vp)], ctypes.c_int),
    "r3d_tsdf_destroy": ([_vp, _vp], ctypes.c_int),
    "r3d_tsdf_reset": ([_vp, _vp], ctypes.c_int),
    "r3d_tsdf_integrate": ([_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, ctypes.POINTER(cloud_ops.DepthCamera), _vp], ctypes.c_int),
    "r3d_tsdf_integrate_f32": _integrate_f32_sig,
    "r3d_tsdf_integrate_f32_dev": _integrate_f32_sig,
    "r3d_tsdf_stats": ([_vp, _vp, ctypes.POINTER(TsdfInfo)], ctypes.c_int),
    "r3d_tsdf_extract_point_cloud": _extract_sig,
    "r3d_tsdf_extract_point_cloud_dev": _extract_sig,
    "r3d_debug_tsdf_units": ([_vp, _vp, _i64, _vp, _vp, _vp, _vp, _i64p], ctypes.c_int),
    "r3d_mesh_from_volume": _mesh_sig,
    "r3d_mesh_from_volume_dev": _mesh_sig,
    "r3d_debug_volume_load_units": ([_vp, _vp, _i64, _vp, _vp, _vp, _vp], ctypes.c_int),
    "r3d_debug_mc_table": ([_vp], ctypes.c_int),
})


def tsdf_params(voxel_length, sdf_trunc, color_type=TSDFVolumeColorType.RGB8, volume_unit_resolution=16, depth_sampling_stride=4, initial_units=0):
    return TsdfParams(float(voxel_length), float(sdf_trunc), int(color_type), int(volume_unit_resolution), int(depth_sampling_stride),
                      int(initial_units))


_ptr = _lib.ptr


def _extrinsic(extrinsic):
    return np.ascontiguousarray(extrinsic, dtype=np.float64).reshape(4, 4)


class ScalableTSDFVolume:
    """ScalableTSDFVolume(voxel_length, sdf_trunc, color_type, volume_unit_resolution=16, depth_sampling_stride=4).  The state
    lives on the device; initial_units (0: the library's default) is the starting capacity of the unit pool, which grows."""

    def __init__(self, voxel_length, sdf_trunc, color_type=TSDFVolumeColorType.RGB8, volume_unit_resolution=16, depth_sampling_stride=4,
                 initial_units=0, ctx=None):
        self.ctx = ctx or _lib.default_context()
        self.voxel_length, self.sdf_trunc, self.color_type = float(voxel_length), float(sdf_trunc), TSDFVolumeColorType(int(color_type))
        self._h = None
        prm = tsdf_params(voxel_length, sdf_trunc, color_type, volume_unit_resolution, depth_sampling_stride, initial_units)
        h = _vp()
        self.ctx.call("r3d_tsdf_create", ctypes.byref(prm), ctypes.byref(h))
        self._h = h

    @property
    def has_color(self):
        return self.color_type == TSDFVolumeColorType.RGB8

    def close(self):
        if getattr(self, "_h", None) and getattr(self.ctx, "_h", None):
            self.ctx.call("r3d_tsdf_destroy", self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def reset(self):
        self.ctx.call("r3d_tsdf_reset", self._h)

    def stats(self):
        st = TsdfInfo()
        self.ctx.call("r3d_tsdf_stats", self._h, ctypes.byref(st))
        return {name: getattr(st, name) for name, _ in TsdfInfo._fields_}

    def __len__(self):
        return int(self.stats()["units"])

    # ---- integrate
    def integrate(self, rgbd, intrinsic, extrinsic):
        """rgbd: a cloud_ops.RGBDImage (raw uint16 depth, its depth_scale and depth_trunc apply; colour in the order given);
        intrinsic: depth_camera(...), a dict with fx / fy / ppx / ppy, a 3x3 matrix or (fx, fy, cx, cy); extrinsic: world -> camera"""
        if not isinstance(rgbd, cloud_ops.RGBDImage):
            raise TypeError("integrate takes a cloud_ops.RGBDImage (cloud_ops.rgbd_image(color, depth, depth_scale, depth_trunc))")
        fx, fy, cx, cy = cloud_ops._intrinsic4(intrinsic)
        H, W = rgbd.depth.shape
        cam = cloud_ops.DepthCamera(fx, fy, cx, cy, rgbd.depth_scale, rgbd.depth_trunc, 0, 0)
        self.ctx.call("r3d_tsdf_integrate", self._h, _ptr(rgbd.depth), _ptr(rgbd.color), W, H, W, W, H, W * rgbd.channels, rgbd.channels,
                      ctypes.byref(cam), _ptr(_extrinsic(extrinsic)))

    def integrate_f32(self, depth, color, intrinsic, extrinsic):
        """depth: float32 [H,W] metres, 0 = no sample; color: uint8 [H,W,3] or None (volumes without colour)"""
        depth = np.ascontiguousarray(depth, dtype=np.float32)
        color = None if color is None else np.ascontiguousarray(color, dtype=np.uint8)
        if depth.ndim != 2 or (color is not None and color.ndim != 3):
            raise ValueError("depth must be [H,W], colour [H,W,channels]")
        fx, fy, cx, cy = cloud_ops._intrinsic4(intrinsic)
        H, W = depth.shape
        ch, cw, cn = color.shape if color is not None else (0, 0, 0)
        self.ctx.call("r3d_tsdf_integrate_f32", self._h, _ptr(depth), _ptr(color), W, H, W, cw, ch, cw * cn, cn, fx, fy, cx, cy,
                      _ptr(_extrinsic(extrinsic)))

    def integrate_device(self, d_depth, d_color, width, height, intrinsic, extrinsic):
        """d_depth: device pointer (int) to contiguous float32 [height][width]; d_color: to uint8 [height][width][3], or None.
        The voxel update is enqueued on the context stream: leave the images alone until the stream has passed."""
        fx, fy, cx, cy = cloud_ops._intrinsic4(intrinsic)
        W, H = int(width), int(height)
        self.ctx.call("r3d_tsdf_integrate_f32_dev", self._h, _vp(d_depth), _vp(d_color), W, H, W, W, H, W * 3, 3, fx, fy, cx, cy,
                      _ptr(_extrinsic(extrinsic)))

    # ---- extract
    def point_count(self):
        n = ctypes.c_int64()
        self.ctx.call("r3d_tsdf_extract_point_cloud", self._h, 0, None, None, None, ctypes.byref(n))
        return n.value

    def extract_arrays(self):
        """-> points, normals, colours (None without colour) as float64 [n,3]"""
        def outputs(n):
            return np.empty((n, 3)), np.empty((n, 3)), np.empty((n, 3)) if self.has_color else None

        _, arrays = self.ctx.count_then_fill("r3d_tsdf_extract_point_cloud", (self._h,), 3, outputs)
        return arrays

    def extract_point_cloud(self):
        xyz, nrm, col = self.extract_arrays()
        return PointCloud(xyz, col, nrm)

    def extract_device(self, d_points, d_normals, d_colors, capacity):
        """r3d_tsdf_extract_point_cloud_dev: device pointers to float64 [capacity][3] arrays -> the number of rows written"""
        n = ctypes.c_int64()
        self.ctx.call("r3d_tsdf_extract_point_cloud_dev", self._h, int(capacity), _vp(d_points), _vp(d_normals), _vp(d_colors), ctypes.byref(n))
        return n.value

    # ---- triangle mesh
    def mesh_counts(self):
        """-> (vertices, triangles) of extract_triangle_mesh()"""
        nv, nt = ctypes.c_int64(), ctypes.c_int64()
        self.ctx.call("r3d_mesh_from_volume", self._h, 0, 0, None, None, None, ctypes.byref(nv), ctypes.byref(nt))
        return nv.value, nt.value

    def extract_triangle_mesh(self):
        """volume.extract_triangle_mesh(): marching cubes on the device -> TriangleMesh (no vertex normals, as in Open3D: call
        compute_vertex_normals()); vertices and triangles in this package's order ("Triangle mesh")"""
        def outputs(nv, nt):
            return np.empty((nv, 3)), np.empty((nv, 3)) if self.has_color else None, np.empty((nt, 3), np.int32)

        _, (vert, col, tri) = self.ctx.count_then_fill("r3d_mesh_from_volume", (self._h,), 3, outputs, n_counts=2)
        return TriangleMesh(vert, tri, col)

    def extract_mesh_device(self, d_vertices, d_colors, d_triangles, cap_vertices, cap_triangles):
        """r3d_mesh_from_volume_dev: device pointers to float64 [cap_vertices][3] (twice) and int32 [cap_triangles][3] arrays ->
        the numbers of vertex and triangle rows written"""
        nv, nt = ctypes.c_int64(), ctypes.c_int64()
        self.ctx.call("r3d_mesh_from_volume_dev", self._h, int(cap_vertices), int(cap_triangles), _vp(d_vertices), _vp(d_colors), _vp(d_triangles),
                      ctypes.byref(nv), ctypes.byref(nt))
        return nv.value, nt.value

    def load_units(self, idx, tsdf, weight, colour=None):
        """the inverse of debug_units(), for the tests: the volume's content becomes these units (keys in any order)"""
        idx = np.ascontiguousarray(idx, dtype=np.int32).reshape(-1, 3)
        n = len(idx)
        tsdf = np.ascontiguousarray(tsdf, dtype=np.float32).reshape(n, UNIT_VOXELS)
        weight = np.ascontiguousarray(weight, dtype=np.float32).reshape(n, UNIT_VOXELS)
        if self.has_color:
            if colour is None:
                raise ValueError("an RGB8 volume needs the colour planes")
            colour = np.ascontiguousarray(colour, dtype=np.float64).reshape(n, 3, UNIT_VOXELS)
        else:
            colour = None
        self.ctx.call("r3d_debug_volume_load_units", self._h, n, _ptr(idx), _ptr(tsdf), _ptr(weight), _ptr(colour))

    def debug_units(self):
        """-> unit indices int32 [n,3] in (X, Y, Z) order, tsdf float32 [n,4096], weight float32 [n,4096], colour float64
        [n,3,4096] (None without colour); voxel (x, y, z) at x*256 + y*16 + z"""
        def outputs(n):
            return (np.empty((n, 3), np.int32), np.empty((n, UNIT_VOXELS), np.float32), np.empty((n, UNIT_VOXELS), np.float32),
                    np.empty((n, 3, UNIT_VOXELS)) if self.has_color else None)

        _, arrays = self.ctx.count_then_fill("r3d_debug_tsdf_units", (self._h,), 4, outputs)
        return arrays


def mc_table():
    """-> the marching-cubes triangle table the library was built with, int8 [256,16] (r3d_debug_mc_table; needs no device)"""
    out = np.empty((256, 16), np.int8)
    rc = _lib.load().r3d_debug_mc_table(_ptr(out))
    if rc != _lib.R3D_OK:
        raise _lib.R3DError(rc, "r3d_debug_mc_table failed")
    return out
