"""CPU-side boundary test of the Fast Global Registration entry points: declared in include/r3d.h, exported by the library, bound
in the ctypes table, with the struct layouts the header states."""
import ctypes
import os
import re

from tests.conftest import ROOT

FGR_SYMBOLS = ("r3d_fgr_correspondence", "r3d_fgr_correspondence_dev", "r3d_fgr_feature_matching", "r3d_fgr_feature_matching_dev",
               "r3d_debug_fgr_tuples", "r3d_debug_fgr_optimize")


def test_fgr_symbols_are_declared_exported_and_bound(r3d):
    src = open(os.path.join(ROOT, "include", "r3d.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(r3d_[a-z0-9_]+)\s*\(", src))
    lib = r3d._lib.load()
    for name in FGR_SYMBOLS:
        assert name in declared, f"{name} is not declared in include/r3d.h"
        assert hasattr(lib, name), f"{name} is not exported by libr3d_hip.so"
        assert name in r3d._lib.exported_symbols(), f"{name} is not in the ctypes table"
        assert getattr(lib, name).argtypes is not None
    assert "r3d_fgr_params" in src and "r3d_fgr_stats" in src


def test_fgr_struct_layouts(r3d):
    assert ctypes.sizeof(r3d.cloud_ops.FgrParams) == 56
    assert ctypes.sizeof(r3d.cloud_ops.FgrStats) == 96
    p = r3d.cloud_ops._fgr_params()
    assert (p.division_factor, p.maximum_correspondence_distance, p.tuple_scale) == (1.4, 0.025, 0.95)
    assert (p.iteration_number, p.maximum_tuple_count, p.use_absolute_scale, p.decrease_mu, p.tuple_test, p.batch) == (64, 1000, 0, 1, 1, 0)
    assert r3d.cloud_ops.FgrParams.seed.offset == 24 and r3d.cloud_ops.FgrParams.batch.offset == 52
    assert r3d.cloud_ops.FgrStats.correspondences.offset == 56 and r3d.cloud_ops.FgrStats.pairs.offset == 88


def test_fgr_public_names(r3d):
    assert r3d.registration_fgr_based_on_correspondence is r3d.cloud_ops.registration_fgr_based_on_correspondence
    assert r3d.registration_fgr_based_on_feature_matching is r3d.cloud_ops.registration_fgr_based_on_feature_matching
    import inspect
    assert inspect.signature(r3d.pointcloud_alignment.global_registration).parameters["method"].default == "ransac"
