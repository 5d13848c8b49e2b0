"""CPU-side tests of the Poisson reconstruction entry points: declared in include/r3d.h, exported by the library, bound in the
ctypes table, named without "tsdf" or "trimesh" (tests/test_tsdf_abi.py and tests/test_trimesh_abi.py pin those sets), refusing a
NULL context before they touch a device; the parameter block's size and defaults; and the Python surface."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from tests.conftest import ROOT

ENTRY_POINTS = ("r3d_poisson_reconstruct", "r3d_poisson_reconstruct_dev", "r3d_debug_poisson_fields", "r3d_debug_poisson_extract")


def test_entry_points_declared_exported_bound_and_refuse_null(r3d):
    lib = r3d._lib.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "r3d.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(r3d_[a-z0-9_]+)\s*\(", header))
    assert {n for n in declared if "poisson" in n} == set(ENTRY_POINTS)
    for name in ENTRY_POINTS:
        assert "tsdf" not in name and "trimesh" not in name
        assert name in r3d._lib.exported_symbols() and hasattr(lib, name)
        fn = getattr(lib, name)
        assert fn.argtypes is not None and fn.restype is ctypes.c_int
        args = [0 if t in (ctypes.c_int32, ctypes.c_int64) else 0.0 if t is ctypes.c_double else None for t in fn.argtypes]
        assert fn(*args) == -1, name


def test_parameter_block(r3d):
    P = r3d.poisson.PoissonParams
    assert ctypes.sizeof(P) == 48
    assert [n for n, _ in P._fields_] == ["depth", "cycles", "pre", "post", "coarse_sweeps", "reserved", "scale", "alpha", "omega"]
    p = r3d.poisson.poisson_params()
    assert (p.depth, p.cycles, p.pre, p.post, p.coarse_sweeps, p.reserved, p.scale, p.alpha, p.omega) == (8, 10, 2, 2, 40, 0, 1.1, 4.0, 0.8)
    header = open(os.path.join(ROOT, "include", "r3d.h")).read()
    block = re.search(r"typedef struct r3d_poisson_params \{(.*?)\} r3d_poisson_params;", header, flags=re.S).group(1)
    block = re.sub(r"/\*.*?\*/", "", block, flags=re.S)
    names = [n.strip() for decl in re.findall(r"(?:int32_t|double)\s+([^;]+);", block) for n in decl.split(",")]
    assert names == [n for n, _ in P._fields_]


def test_python_surface(r3d):
    fn = r3d.create_from_point_cloud_poisson
    assert fn is r3d.poisson.create_from_point_cloud_poisson
    sig = inspect.signature(fn)
    assert list(sig.parameters) == ["pcd", "depth", "width", "scale", "linear_fit", "n_threads", "cycles", "alpha", "ctx"]
    assert [sig.parameters[n].default for n in list(sig.parameters)[1:]] == [8, 0, 1.1, False, -1, 10, 4.0, None]
    assert callable(r3d.TriangleMesh.create_from_point_cloud_poisson)
    rm = inspect.signature(r3d.pipeline.reconstruct_mesh)
    assert list(rm.parameters) == ["cloud", "depth", "smooth_iterations", "ctx"]
    assert (rm.parameters["depth"].default, rm.parameters["smooth_iterations"].default) == (6, 5)
    stage = r3d.mesh_reconstruction.MeshReconstruction()
    assert r3d.MeshReconstruction is r3d.mesh_reconstruction.MeshReconstruction and callable(stage.reconstruct_mesh)
    assert (stage.depth, stage.smooth_iterations) == (6, 5)


def test_python_refusals_need_no_device(r3d):
    """what the Python layer turns down before any library call"""
    cloud = r3d.PointCloud(np.zeros((4, 3)), normals=np.ones((4, 3)))
    with pytest.raises(r3d.R3DError) as e:
        r3d.create_from_point_cloud_poisson(cloud, depth=5, width=1)
    assert e.value.code == -4
    with pytest.raises(r3d.R3DError) as e:
        r3d.create_from_point_cloud_poisson(cloud, depth=5, linear_fit=True)
    assert e.value.code == -4
    with pytest.raises(r3d.R3DError) as e:
        r3d.TriangleMesh.create_from_point_cloud_poisson(r3d.PointCloud(np.zeros((4, 3))), depth=5)
    assert e.value.code == -1
