"""CPU-side boundary tests of the RGB-D odometry entry points: struct layouts as include/r3d.h states them, and every entry
point refuses a NULL context before it touches a device."""
import ctypes

ENTRY_POINTS = ("r3d_rgbd_odometry", "r3d_rgbd_odometry_f32", "r3d_rgbd_odometry_f32_dev", "r3d_debug_rgbd_convert",
                "r3d_debug_rgbd_prepare", "r3d_debug_rgbd_iteration")


def test_struct_sizes(r3d):
    assert ctypes.sizeof(r3d.cloud_ops.OdometryParams) == 48
    assert ctypes.sizeof(r3d.cloud_ops.OdometryStats) == 56
    p = r3d.cloud_ops.odometry_params()
    assert (p.depth_diff_max, p.depth_min, p.depth_max, list(p.iterations), p.levels, p.jacobian) == (0.03, 0.0, 4.0, [20, 10, 5, 0], 3, 0)
    assert r3d.cloud_ops.odometry_params("color", iteration_number_per_pyramid_level=(7,)).levels == 1


def test_null_context_is_badarg(r3d):
    lib = r3d._lib.load()
    for name in ENTRY_POINTS:
        fn = getattr(lib, name)
        args = [0 if t in (ctypes.c_int32, ctypes.c_int64) else 0.0 if t is ctypes.c_double else None for t in fn.argtypes]
        assert fn(*args) == -1, name
