"""CPU-side tests of the triangle-mesh entry points: declared in include/r3d.h, exported by the library, bound in the ctypes table,
named without "tsdf" (tests/test_tsdf_abi.py pins that set), and refusing a NULL context before they touch a device; plus the
host-side members TriangleMesh gains."""
import ctypes
import os
import re

import numpy as np

from tests.conftest import ROOT

ENTRY_POINTS = ("r3d_trimesh_incidence", "r3d_trimesh_adjacency", "r3d_trimesh_smooth", "r3d_trimesh_smooth_dev", "r3d_trimesh_normals",
                "r3d_trimesh_normals_dev", "r3d_trimesh_compact", "r3d_trimesh_compact_dev")


def test_entry_points_declared_exported_bound_and_refuse_null(r3d):
    lib = r3d._lib.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "r3d.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(r3d_[a-z0-9_]+)\s*\(", header))
    assert {n for n in declared if "trimesh" in n} == set(ENTRY_POINTS)
    for name in ENTRY_POINTS:
        assert "tsdf" not in name
        assert name in r3d._lib.exported_symbols() and hasattr(lib, name)
        fn = getattr(lib, name)
        assert fn.argtypes is not None and fn.restype is ctypes.c_int
        args = [0 if t in (ctypes.c_int32, ctypes.c_int64) else 0.0 if t is ctypes.c_double else None for t in fn.argtypes]
        assert fn(*args) == -1, name


def test_constants_match_the_header(r3d):
    header = open(os.path.join(ROOT, "include", "r3d.h")).read()
    values = {k: int(v) for k, v in re.findall(r"#define (R3D_(?:SMOOTH|SCOPE|NORMALS|COMPACT)_[A-Z_]+) (\d+)", header)}
    mo = r3d.mesh_ops
    assert (values["R3D_SMOOTH_SIMPLE"], values["R3D_SMOOTH_LAPLACIAN"], values["R3D_SMOOTH_TAUBIN"]) == (mo.SMOOTH_SIMPLE, mo.SMOOTH_LAPLACIAN, mo.SMOOTH_TAUBIN)
    assert {s.name.upper(): int(s) for s in r3d.FilterScope} == {k[len("R3D_SCOPE_"):]: v for k, v in values.items() if k.startswith("R3D_SCOPE_")}
    assert (values["R3D_COMPACT_DROP_DEGENERATE"], values["R3D_COMPACT_DROP_UNREFERENCED"], values["R3D_COMPACT_DROP_NON_FINITE"]) == \
        (mo.DROP_DEGENERATE, mo.DROP_UNREFERENCED, mo.DROP_NON_FINITE)
    assert values["R3D_NORMALS_RAW"] == mo.NORMALS_RAW
    assert r3d.FilterScope is mo.FilterScope


def test_triangle_mesh_gains_its_members(r3d):
    mesh = r3d.TriangleMesh(np.zeros((3, 3)), [[0, 1, 2]])
    assert mesh.triangle_normals is None and mesh.adjacency_list is None
    assert not mesh.has_triangle_normals() and not mesh.has_adjacency_list()
    for name in ("filter_smooth_simple", "filter_smooth_laplacian", "filter_smooth_taubin", "compute_triangle_normals", "compute_adjacency_list",
                 "remove_degenerate_triangles", "remove_unreferenced_vertices", "remove_vertices_by_mask", "remove_triangles_by_mask",
                 "remove_non_finite_vertices"):
        assert callable(getattr(mesh, name)), name
    assert callable(r3d.pipeline.mesh_postprocess)
    # the host helper is unchanged by default
    assert np.array_equal(mesh.compute_vertex_normals().vertex_normals, np.zeros((3, 3)))
