"""CPU-side boundary tests of the TSDF volume entry points: struct layouts as include/r3d.h states them, and every entry point
refuses a NULL context before it touches a device."""
import ctypes

ENTRY_POINTS = ("r3d_tsdf_create", "r3d_tsdf_destroy", "r3d_tsdf_reset", "r3d_tsdf_integrate", "r3d_tsdf_integrate_f32",
                "r3d_tsdf_integrate_f32_dev", "r3d_tsdf_stats", "r3d_tsdf_extract_point_cloud", "r3d_tsdf_extract_point_cloud_dev",
                "r3d_debug_tsdf_units")


def test_struct_sizes_and_defaults(r3d):
    assert ctypes.sizeof(r3d.tsdf.TsdfParams) == 32
    assert ctypes.sizeof(r3d.tsdf.TsdfInfo) == 48
    p = r3d.tsdf.tsdf_params(0.01, 0.04)
    assert (p.voxel_length, p.sdf_trunc, p.color_type, p.volume_unit_resolution, p.depth_sampling_stride, p.initial_units) == \
        (0.01, 0.04, 1, 16, 4, 0)
    assert (int(r3d.TSDFVolumeColorType.NoColor), int(r3d.TSDFVolumeColorType.RGB8)) == (0, 1)
    assert r3d.tsdf.tsdf_params(0.01, 0.04, r3d.TSDFVolumeColorType.NoColor, depth_sampling_stride=2, initial_units=8).initial_units == 8


def test_every_entry_point_is_in_the_table(r3d):
    assert set(ENTRY_POINTS) == {n for n in r3d._lib.exported_symbols() if "tsdf" in n}


def test_null_context_is_badarg(r3d):
    lib = r3d._lib.load()
    for name in ENTRY_POINTS:
        fn = getattr(lib, name)
        args = [0 if t in (ctypes.c_int32, ctypes.c_int64) else 0.0 if t is ctypes.c_double else None for t in fn.argtypes]
        assert fn(*args) == -1, name
