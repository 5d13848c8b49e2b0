"""CPU-side tests of the triangle-mesh entry points and of TriangleMesh: the entry points are in the ctypes table and refuse a
NULL context or a NULL table before they touch a device; the mesh class's host-side members."""
import ctypes

import numpy as np

CONTEXT_ENTRY_POINTS = ("r3d_mesh_from_volume", "r3d_mesh_from_volume_dev", "r3d_debug_volume_load_units")


def test_entry_points_are_in_the_table_and_refuse_null(r3d):
    lib = r3d._lib.load()
    for name in CONTEXT_ENTRY_POINTS + ("r3d_debug_mc_table",):
        assert name in r3d._lib.exported_symbols()
    for name in CONTEXT_ENTRY_POINTS:
        fn = getattr(lib, name)
        args = [0 if t in (ctypes.c_int32, ctypes.c_int64) else None for t in fn.argtypes]
        assert fn(*args) == -1, name
    assert lib.r3d_debug_mc_table(None) == -1


def test_mc_table_needs_no_device(r3d):
    table = r3d.tsdf.mc_table()
    assert table.shape == (256, 16) and table.dtype == np.int8
    assert table.min() == -1 and table.max() == 11 and int((table >= 0).sum()) == 3 * 820
    assert np.array_equal(table, r3d.tsdf.mc_table())


def test_triangle_mesh_members(r3d):
    assert r3d.TriangleMesh is r3d.pointcloud.TriangleMesh
    empty = r3d.TriangleMesh()
    assert empty.vertices.shape == (0, 3) and empty.triangles.shape == (0, 3) and empty.triangles.dtype == np.int32
    assert not (empty.has_vertices() or empty.has_triangles() or empty.has_vertex_colors() or empty.has_vertex_normals())
    assert empty.compute_vertex_normals().vertex_normals.shape == (0, 3)
    # a tetrahedron with outward faces, and a fifth vertex no triangle uses: its normal stays zero
    vert = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [5, 5, 5]], np.float64)
    tri = [[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]]
    mesh = r3d.TriangleMesh(vert, tri, vertex_colors=np.full((5, 3), 0.5))
    assert mesh.has_vertices() and mesh.has_triangles() and mesh.has_vertex_colors() and not mesh.has_vertex_normals()
    assert mesh.triangles.dtype == np.int32 and mesh.vertex_normals is None
    n = mesh.compute_vertex_normals().vertex_normals
    assert mesh.has_vertex_normals()
    # vertex 0: faces (0,0,-1) + (0,-1,0) + (-1,0,0); vertex 1: (0,0,-1) + (0,-1,0) + (1,1,1)
    assert np.allclose(n[0], -np.ones(3) / np.sqrt(3.0)) and np.allclose(n[1], np.array([1.0, 0.0, 0.0]))
    assert np.array_equal(n[4], np.zeros(3))
    assert np.allclose(np.sqrt((n[:4] ** 2).sum(1)), 1.0)
