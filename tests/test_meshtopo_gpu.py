"""GPU tests of the mesh-topology operations (csrc/meshtopo.hip, the sort wrapper of csrc/cloud.hip, mesh_ops.py, TriangleMesh) against
the numpy restatement of tests/meshtopo_ref.py, which tests/test_meshtopo_ref.py holds equal to its literal form on the CPU.

Everything is compared bit for bit: the tables, labels and maps are integers, and a cluster's area is a fixed sequence of IEEE
subtract, multiply, add and square root in float64 (the build has -ffp-contract=off) added in the shape the restatement writes."""
import ctypes

import numpy as np
import pytest

from tests import meshtopo_cases as mc
from tests import meshtopo_ref as mr
from tests import trimesh_cases as tc

pytestmark = pytest.mark.gpu

_vp = ctypes.c_void_p
ALL_CASES = {**mc.CASES, **mc.BIG_CASES}
ALL_WELDS = {**mc.WELD_CASES, **mc.WELD_BIG, **mc.TRIANGLE_CASES}
NAMES = ("vertices", "triangles", "normals", "colours", "vertex_map", "triangle_origin")


def _bits(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if got.tobytes() != want.tobytes():
        differ = got.view(np.uint64) != want.view(np.uint64) if got.dtype == np.float64 else got != want
        bad = np.flatnonzero(differ.reshape(len(got), -1).any(1)) if len(got) else []
        raise AssertionError(f"{what}: {len(bad)} of {len(got)} rows differ, first {bad[:5]}: {got[bad[:3]]} against {want[bad[:3]]}")


def _code(fn, *args, **kw):
    with pytest.raises(Exception) as e:
        fn(*args, **kw)
    assert hasattr(e.value, "code") and str(e.value).split(":", 1)[1].strip(), "no message came through r3d_last_error"
    return e.value.code


def _p(a):
    return None if a is None else a.ctypes.data_as(_vp)


# ---- the sort alone ------------------------------------------------------------------------------------------------------------------
def _sorted(keys, values=None):
    order = np.argsort(keys, kind="stable")
    return keys[order], (order if values is None else values[order]).astype(np.int32)


@pytest.mark.parametrize("n", (1, 63, 64, 65, 1023, 1024, 1025, 4097, 262_145))
def test_sort_pairs(r3d, n):
    """keys below 2^bits for 1, 2, 3, 6 and 8 passes (odd and even numbers of buffer swaps); equal keys keep ascending values"""
    rng = np.random.default_rng(n)
    sort = r3d.mesh_ops.sort_pairs_u64
    for bits in (8, 16, 17, 42, 64):
        keys = rng.integers(0, 2 ** 63, n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, n, dtype=np.uint64)
        keys >>= np.uint64(64 - bits)
        if n > 1000:
            keys[rng.integers(0, n, n // 2)] = keys[0]             # long runs of one key
        got = sort(keys, bits)
        want = _sorted(keys)
        _bits(got[0], want[0], f"keys, {bits} bits")
        _bits(got[1], want[1], f"values, {bits} bits")
        values = rng.permutation(n).astype(np.int32)                # given values travel with their keys
        got = sort(keys, bits, values)
        _bits(got[1], _sorted(keys, values)[1], f"given values, {bits} bits")
    same = np.full(n, 0x0123456789ABCDEF, np.uint64)
    got = sort(same, 64)
    _bits(got[0], same, "equal keys")
    _bits(got[1], np.arange(n, dtype=np.int32), "equal keys keep ascending values")
    for byte in range(8):                                           # keys that differ in exactly one byte
        keys = same ^ (rng.integers(0, 256, n, dtype=np.uint64) << np.uint64(8 * byte))
        got = sort(keys, 64)
        want = _sorted(keys)
        _bits(got[0], want[0], f"keys differing in byte {byte}")
        _bits(got[1], want[1], f"values, keys differing in byte {byte}")


def test_sort_pairs_protocol(r3d):
    k, v = r3d.mesh_ops.sort_pairs_u64(np.zeros(0, np.uint64))
    assert len(k) == 0 and len(v) == 0
    assert _code(r3d.mesh_ops.sort_pairs_u64, np.zeros(4, np.uint64), 65) == -1
    assert _code(r3d.mesh_ops.sort_pairs_u64, np.zeros(4, np.uint64), -1) == -1


# ---- edge table and components -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ALL_CASES))
def test_edge_table_and_components_bit_for_bit(r3d, name):
    vert, tri = ALL_CASES[name]()
    mo = r3d.mesh_ops
    for got, want, what in zip(mo.edges(len(vert), tri), mr.edges(len(vert), tri), ("edges", "counts", "stats")):
        _bits(got, want, what)
    for got, want, what in zip(mo.components(vert, tri), mr.components(vert, tri), ("triangle_clusters", "cluster_n_triangles", "cluster_area")):
        _bits(got, want, what)


@pytest.mark.parametrize("name", ("islands", "book1025"))
def test_components_device_form_equals_host_form(r3d, name):
    vert, tri = mc.CASES[name]()
    mo, ctx = r3d.mesh_ops, r3d._lib.default_context()
    labels, count, area = mo.components(vert, tri)
    ncl = len(count)
    d = [ctx.to_device(vert), ctx.to_device(tri), ctx.alloc(4 * len(tri)), ctx.alloc(8 * ncl), ctx.alloc(8 * ncl)]
    try:
        assert mo.components_device(d[0], d[1], len(vert), len(tri), d[2]) == ncl                     # labels alone
        got = np.empty(len(tri), np.int32)
        ctx.d2h(got, d[2])
        _bits(got, labels, "labels, capacity 0")
        assert mo.components_device(d[0], d[1], len(vert), len(tri), d[2], ncl, d[3], d[4]) == ncl
        got_n, got_a = np.empty(ncl, np.int64), np.empty(ncl)
        ctx.d2h(got, d[2])
        ctx.d2h(got_n, d[3])
        ctx.d2h(got_a, d[4])
        _bits(got, labels, "labels")
        _bits(got_n, count, "counts")
        _bits(got_a, area, "areas")
        assert _code(mo.components_device, d[0], d[1], len(vert), len(tri), d[1]) == -1                # labels over the triangles
        assert _code(mo.components_device, d[0], d[1], len(vert), len(tri), d[2], ncl, d[3], d[3]) == -1
    finally:
        for p in d:
            ctx.free(p)


# ---- welds ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ALL_WELDS))
def test_welds_bit_for_bit(r3d, name):
    vert, tri, nrm, col = ALL_WELDS[name]()
    mo = r3d.mesh_ops
    for flags in (mo.DEDUP_VERTICES, mo.DEDUP_TRIANGLES, mo.DEDUP_VERTICES | mo.DEDUP_TRIANGLES):
        for a_n, a_c in ((nrm, col), (None, None)) if flags != mo.DEDUP_TRIANGLES else ((None, col),):
            got = mo.dedup(vert, tri, flags, a_n, a_c)
            want = mr.dedup(vert, tri, flags, a_n, a_c)
            for g, w, what in zip(got, want, NAMES):
                assert (g is None) == (w is None), what
                if g is not None:
                    _bits(g, w, f"{what}, flags {flags}")


def test_triangle_duplicates_of_the_doubled_big_grid(r3d):
    vert, tri = mc.doubled_big_grid()
    got = r3d.mesh_ops.dedup(vert, tri, r3d.mesh_ops.DEDUP_TRIANGLES)
    want = mr.dedup(vert, tri, mr.DEDUP_TRIANGLES)
    for g, w, what in zip(got, want, NAMES):
        if w is not None:
            _bits(g, w, what)


def test_dedup_device_form_equals_host_form(r3d):
    vert, tri, nrm, col = mc.TRIANGLE_CASES["twice_grid"]()
    mo, ctx = r3d.mesh_ops, r3d._lib.default_context()
    want = mo.dedup(vert, tri, 3, nrm, col)
    nv, nt = len(vert), len(tri)
    kv, kt = len(want[0]), len(want[1])
    d_in = [ctx.to_device(a) for a in (vert, tri, nrm, col)]
    d_out = [ctx.alloc(24 * kv), ctx.alloc(12 * kt), ctx.alloc(24 * kv), ctx.alloc(24 * kv), ctx.alloc(4 * nv), ctx.alloc(4 * kt)]
    try:
        assert mo.dedup_device(d_in[0], d_in[1], nv, nt, 3, 0, 0, None, None) == (kv, kt)
        kw = dict(d_normals=d_in[2], d_colors=d_in[3], d_out_normals=d_out[2], d_out_colors=d_out[3], d_vertex_map=d_out[4], d_triangle_origin=d_out[5])
        assert mo.dedup_device(d_in[0], d_in[1], nv, nt, 3, kv, kt, d_out[0], d_out[1], **kw) == (kv, kt)
        for p, w, what in zip(d_out, want, NAMES):
            got = np.empty_like(w)
            ctx.d2h(got, p)
            _bits(got, w, what)
        assert _code(mo.dedup_device, d_in[0], d_in[1], nv, nt, 3, kv, kt, d_in[0], d_out[1]) == -1                    # output over an input
        assert _code(mo.dedup_device, d_in[0], d_in[1], nv, nt, 3, kv, kt, d_out[0], d_out[1], d_vertex_map=d_out[0]) == -1   # two outputs overlap
        assert _code(mo.dedup_device, d_in[0], d_in[1], nv, nt, 3, kv - 1, kt, d_out[0], d_out[1]) == -1
    finally:
        for p in d_in + d_out:
            ctx.free(p)


# ---- protocols -----------------------------------------------------------------------------------------------------------------------
def test_count_capacity_and_refusals(r3d):
    vert, tri, nrm, col = mc.messy()
    nv, nt = len(vert), len(tri)
    ctx, lib = r3d._lib.default_context(), r3d._lib.load()
    n, stats = ctypes.c_int64(), np.zeros(4, np.int64)
    ctx.call("r3d_meshtopo_edges", nv, nt, _p(tri), 0, None, None, _p(stats), ctypes.byref(n))          # a count-only call
    assert n.value == 11 and stats.tolist() == [11, 6, 2, 1]
    edg, cnt = np.full((11, 2), -7, np.int32), np.full(11, -7, np.int32)
    assert lib.r3d_meshtopo_edges(ctx._h, nv, nt, _p(tri), 10, _p(edg), _p(cnt), None, ctypes.byref(n)) == -1   # a capacity one short
    assert n.value == 11 and (edg == -7).all() and (cnt == -7).all() and lib.r3d_last_error(ctx._h)
    labels, ncl = np.full(nt, -7, np.int32), ctypes.c_int64()
    ctx.call("r3d_meshtopo_components", nv, nt, None, _p(tri), 0, _p(labels), None, None, ctypes.byref(ncl))   # labels need no vertices
    assert ncl.value == 2 and labels.min() == 0
    count, area = np.full(1, -7, np.int64), np.full(1, -7.0)
    labels[:] = -7
    assert lib.r3d_meshtopo_components(ctx._h, nv, nt, _p(vert), _p(tri), 1, _p(labels), _p(count), _p(area), ctypes.byref(ncl)) == -1
    assert ncl.value == 2 and (labels == -7).all() and count[0] == -7 and area[0] == -7.0 and lib.r3d_last_error(ctx._h)
    kv, kt = ctypes.c_int64(), ctypes.c_int64()
    ov, ot = np.full((nv, 3), -7.0), np.full((nt, 3), -7, np.int32)
    args = (ctx._h, nv, nt, _p(vert), None, None, _p(tri), 2)
    assert lib.r3d_meshtopo_dedup(*args, nv, nt - 2, _p(ov), None, None, _p(ot), None, None, ctypes.byref(kv), ctypes.byref(kt)) == -1
    assert (kv.value, kt.value) == (nv, nt - 1) and (ov == -7.0).all() and (ot == -7).all() and lib.r3d_last_error(ctx._h)
    mo = r3d.mesh_ops
    for bad in (nv, -1):                                              # an index equal to nv and an index of -1
        broken = np.array(tri)
        broken[3, 1] = bad
        assert _code(mo.edges, nv, broken) == -1
        assert _code(mo.components, vert, broken) == -1
        for flags in (1, 2, 3):
            assert _code(mo.dedup, vert, broken, flags) == -1
    assert _code(mo.dedup, vert, tri, 4) == -1 and _code(mo.dedup, vert, tri, -1) == -1                 # unknown flags
    assert _code(mo.edges, 0, tri) == -1                                                                # triangles without vertices


def test_empty_meshes(r3d):
    mo = r3d.mesh_ops
    none_v, none_t = np.zeros((0, 3)), np.zeros((0, 3), np.int32)
    for vert in (none_v, tc.tetrahedron()[0]):
        edg, cnt, stats = mo.edges(len(vert), none_t)
        assert edg.shape == (0, 2) and len(cnt) == 0 and not stats.any()
        labels, count, area = mo.components(vert, none_t)
        assert len(labels) == 0 and len(count) == 0 and len(area) == 0
        for flags in (1, 2, 3):
            got = mo.dedup(vert, none_t, flags)
            want = mr.dedup(vert, none_t, flags)
            for g, w, what in zip(got, want, NAMES):
                if w is not None:
                    _bits(g, w, what)


# ---- TriangleMesh end to end -----------------------------------------------------------------------------------------------------------
def test_remove_small_components(r3d):
    vert, tri = mc.islands()
    nrm, col = tc.attributes(len(vert), 21)
    mesh = r3d.TriangleMesh(vert, tri, col, nrm)
    labels, count, area = mesh.cluster_connected_triangles()
    assert len(count) == 54
    mesh.remove_small_components(min_triangles=100)
    _, kept, _ = mesh.cluster_connected_triangles()
    assert sorted(kept.tolist()) == [720, 720, 4554, 4692]                       # the two half-grids and the two spheres
    gone = mr.component_mask(labels, count, area, min_triangles=100)
    from tests import trimesh_ref as tr                                          # the restatement of the compaction
    want = tr.compact(vert, tri, tr.DROP_UNREFERENCED, triangle_keep=~gone, normals=nrm, colors=col)
    _bits(mesh.vertices, want[0], "vertices")
    _bits(mesh.triangles, want[1], "triangles")
    _bits(mesh.vertex_normals, want[2], "normals")
    _bits(mesh.vertex_colors, want[3], "colours")
    mesh = r3d.TriangleMesh(vert, tri).remove_small_components(keep_largest=True)
    assert len(mesh.triangles) == 4692 and len(mesh.vertices) == 35 * 70 and mesh.is_edge_manifold()
    assert mesh.cluster_connected_triangles()[1].tolist() == [4692]


def test_edge_queries_and_welds_of_triangle_mesh(r3d):
    vert, tri = tc.tsdf_sphere()
    mesh = r3d.TriangleMesh(vert, tri)
    assert mesh.euler_poincare_characteristic() == 2 and mesh.is_edge_manifold(allow_boundary_edges=False)
    both = mesh + r3d.TriangleMesh(vert + [40.0, 0, 0], tri)
    assert both.euler_poincare_characteristic() == 4 and len(both.cluster_connected_triangles()[1]) == 2
    assert len(both.get_non_manifold_edges()) == 0 and len(both.get_non_manifold_edges(allow_boundary_edges=False)) == 0
    vert, tri = tc.messy()
    mesh = r3d.TriangleMesh(vert, tri)
    _bits(mesh.get_non_manifold_edges(), mr.non_manifold_edges(len(vert), tri), "non-manifold edges")
    _bits(mesh.get_non_manifold_edges(False), mr.non_manifold_edges(len(vert), tri, False), "edges whose count is not 2")
    assert not mesh.is_edge_manifold() and mesh.euler_poincare_characteristic() == 3
    vert, tri = tc.two_triangles()
    assert r3d.TriangleMesh(vert, tri).is_edge_manifold() and not r3d.TriangleMesh(vert, tri).is_edge_manifold(allow_boundary_edges=False)
    # mesh + mesh welds back to the mesh, attributes and triangle normals of the first occurrences included
    vert, tri = tc.noisy_sphere()
    nrm, col = tc.attributes(len(vert), 22)
    one = r3d.TriangleMesh(vert, tri, col, nrm).compute_triangle_normals()
    two = one + one
    two.adjacency_list = []
    assert two.remove_duplicated_vertices() is two and len(two.vertices) == len(vert) and len(two.triangles) == 2 * len(tri)
    assert two.remove_duplicated_triangles() is two and two.adjacency_list is None
    _bits(two.vertices, np.asarray(vert), "vertices")
    _bits(two.triangles, np.asarray(tri), "triangles")
    _bits(two.vertex_normals, nrm, "normals")
    _bits(two.vertex_colors, col, "colours")
    _bits(two.triangle_normals, one.triangle_normals, "triangle normals follow triangle_origin")


def test_mesh_postprocess_default_is_unchanged_and_keywords_apply(r3d):
    vert, tri = tc.tsdf_sphere()
    col = tc.tsdf_sphere_colours()
    mesh = r3d.TriangleMesh(vert, tri, col)
    out = r3d.pipeline.mesh_postprocess(mesh)
    want = mesh.filter_smooth_laplacian(5, 0.5)                                    # the parent commit's sequence, by hand
    want.remove_degenerate_triangles().remove_non_finite_vertices().remove_unreferenced_vertices()
    want.compute_vertex_normals(device=True)
    for name in ("vertices", "triangles", "vertex_colors", "vertex_normals"):
        _bits(getattr(out, name), getattr(want, name), name)
    two = mesh + r3d.TriangleMesh(vert + [40.0, 0, 0], tri[:50], col) + mesh
    out = r3d.pipeline.mesh_postprocess(two, 0, weld=True, keep_largest_component=True)
    assert len(out.vertices) == len(vert) and len(out.triangles) == len(tri) and out.euler_poincare_characteristic() == 2
    out = r3d.pipeline.mesh_postprocess(two, 0, min_component_triangles=51)
    assert len(out.triangles) == 2 * len(tri)
