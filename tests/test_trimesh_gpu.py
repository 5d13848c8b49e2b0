"""GPU tests of the triangle-mesh operations (csrc/trimesh.hip, mesh_ops.py, TriangleMesh) against the numpy restatement of
tests/trimesh_ref.py, which tests/test_trimesh_ref.py holds equal to its literal form on the CPU.

Everything is compared bit for bit: the lists are integers, and every floating-point result is a fixed sequence of IEEE add,
subtract, multiply, divide and square root in float64 (the build has -ffp-contract=off), in the order the restatement writes."""
import ctypes

import numpy as np
import pytest

from tests import trimesh_cases as tc
from tests import trimesh_ref as tr

pytestmark = pytest.mark.gpu

_vp = ctypes.c_void_p
KINDS = (tr.SIMPLE, tr.LAPLACIAN, tr.TAUBIN)
FILTER_CASES = ("two_triangles", "messy", "fan33", "fan65", "fan5000", "grid70x70", "noisy_sphere", "tsdf_sphere")


def _bits(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if got.tobytes() != want.tobytes():
        bad = np.flatnonzero((got != want).reshape(len(got), -1).any(1)) if len(got) else []
        raise AssertionError(f"{what}: {len(bad)} of {len(got)} rows differ, first {bad[:5]}: {got[bad[:3]]} against {want[bad[:3]]}")


def _code(fn, *args):
    with pytest.raises(Exception) as e:
        fn(*args)
    assert hasattr(e.value, "code") and str(e.value).split(":", 1)[1].strip(), "no message came through r3d_last_error"
    return e.value.code


def _p(a):
    return None if a is None else a.ctypes.data_as(_vp)


# ---- lists ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(tc.CASES))
def test_incidence_and_adjacency_entry_by_entry(r3d, name):
    vert, tri = tc.CASES[name]()
    mo = r3d.mesh_ops
    off, corners = mo.incidence(len(vert), tri)
    want_off, want = tr.incidence(len(vert), tri)
    _bits(off, want_off, "incidence offsets")
    _bits(corners, want, "corners")
    off, nbs = mo.adjacency(len(vert), tri)
    want_off, want = tr.adjacency(len(vert), tri)
    _bits(off, want_off, "adjacency offsets")
    _bits(nbs, want, "neighbours")


def test_million_vertex_grid(r3d):
    """past 256 scan tiles: the lists and one Laplacian step"""
    vert, tri = tc.big_grid()
    mo = r3d.mesh_ops
    nv = len(vert)
    off, corners = mo.incidence(nv, tri)
    want_off, want = tr.incidence(nv, tri)
    _bits(off, want_off, "incidence offsets")
    _bits(corners, want, "corners")
    off, nbs = mo.adjacency(nv, tri)
    want_off, want = tr.adjacency(nv, tri)
    _bits(off, want_off, "adjacency offsets")
    _bits(nbs, want, "neighbours")
    got = mo.smooth(vert, tri, mo.SMOOTH_LAPLACIAN, 1)[0]
    _bits(got, tr.step(tr.LAPLACIAN, vert, [np.asarray(vert)], want_off, want, 0.5)[0], "Laplacian step")


# ---- filters -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FILTER_CASES)
@pytest.mark.parametrize("kind", KINDS)
def test_filters_bit_for_bit(r3d, name, kind):
    """1, 2 and 5 iterations (odd and even numbers of buffer swaps), every scope, with and without normals and colours.
    filter_smooth_simple uses add and divide only; the Laplacian and Taubin steps add subtract, multiply and the float64 square
    root, all correctly rounded, so they are held bit for bit as well"""
    vert, tri = tc.CASES[name]()
    nrm, col = tc.attributes(len(vert), 11)
    mo = r3d.mesh_ops
    for n in (1, 2, 5):
        for scope in (tr.ALL, tr.COLOR, tr.NORMAL, tr.VERTEX):
            for a_n, a_c in ((nrm, col), (None, None), (None, col)):
                got = mo.smooth(vert, tri, kind, n, 0.5, -0.53, scope, a_n, a_c)
                want = tr.smooth(kind, vert, tri, n, 0.5, -0.53, scope, a_n, a_c)
                for g, w, what in zip(got, want, ("vertices", "normals", "colours")):
                    assert (g is None) == (w is None)
                    if g is not None:
                        _bits(g, w, f"{what} after {n} iterations, scope {scope}")
    got = mo.smooth(vert, tri, kind, 3, 0.3, -0.31, tr.ALL, nrm, col)          # other factors than the defaults
    for g, w in zip(got, tr.smooth(kind, vert, tri, 3, 0.3, -0.31, tr.ALL, nrm, col)):
        _bits(g, w, "lambda 0.3, mu -0.31")


def test_zero_iterations_copy(r3d):
    vert, tri = tc.noisy_sphere()
    nrm, col = tc.attributes(len(vert), 12)
    for kind in KINDS:
        got = r3d.mesh_ops.smooth(vert, tri, kind, 0, normals=nrm, colors=col)
        for g, w in zip(got, (vert, nrm, col)):
            _bits(g, w, "n == 0")
            assert not np.shares_memory(g, w)


def test_coincident_neighbour_and_isolated_vertex(r3d):
    """a vertex at the position of one of its neighbours: distance 0, weight 1e12; a vertex without a triangle is kept"""
    vert, tri = tc.noisy_sphere()
    vert = np.array(vert)
    off, nbs = tr.adjacency(len(vert), tri)
    vert[nbs[off[17]]] = vert[17]
    for kind in (tr.LAPLACIAN, tr.TAUBIN):
        _bits(r3d.mesh_ops.smooth(vert, tri, kind, 2)[0], tr.smooth(kind, vert, tri, 2)[0], "coincident")
    assert np.isfinite(r3d.mesh_ops.smooth(vert, tri, tr.LAPLACIAN, 2)[0]).all()
    vert, tri = tc.messy()
    iso = int(np.flatnonzero((vert == tc.MESSY_ISOLATED).all(1))[0])
    nrm, col = tc.attributes(len(vert), 13)
    for kind in KINDS:
        got = r3d.mesh_ops.smooth(vert, tri, kind, 3, normals=nrm, colors=col)
        assert np.array_equal(got[0][iso], tc.MESSY_ISOLATED) and np.array_equal(got[1][iso], nrm[iso]) and np.array_equal(got[2][iso], col[iso])
        assert all(np.isfinite(g).all() for g in got)


@pytest.mark.parametrize("kind", (tr.SIMPLE, tr.LAPLACIAN))
def test_nan_poisons_one_ring_per_step(r3d, kind):
    vert, tri = tc.grid(70, 70)
    vert = np.array(vert)
    seed = int(np.flatnonzero((np.abs(vert[:, 0] - 35) < 0.5) & (np.abs(vert[:, 1] - 35) < 0.5))[0])
    vert[seed, 1] = np.nan
    for n in (1, 2, 3):
        got = r3d.mesh_ops.smooth(vert, tri, kind, n)[0]
        want = tr.smooth(kind, vert, tri, n)[0]
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan) and 0 < nan.any(1).sum() < 60
        _bits(np.where(nan, 0.0, got), np.where(nan, 0.0, want), f"beside the NaN ring after {n} steps")


# ---- normals -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("tetrahedron", "messy", "fan4097", "grid64x64", "noisy_sphere", "tsdf_sphere"))
def test_normals_bit_for_bit(r3d, name):
    vert, tri = tc.CASES[name]()
    mo = r3d.mesh_ops
    _bits(mo.vertex_normals(vert, tri, raw=True), tr.vertex_normals(vert, tri, raw=True), "unnormalised vertex sums")
    _bits(mo.triangle_normals(vert, tri, raw=True), tr.triangle_normals(vert, tri, raw=True), "cross products")
    _bits(mo.vertex_normals(vert, tri), tr.vertex_normals(vert, tri), "vertex normals")
    _bits(mo.triangle_normals(vert, tri), tr.triangle_normals(vert, tri), "triangle normals")


def test_vertex_normals_equal_the_numpy_helper_on_the_sphere(r3d):
    vert, tri = tc.tsdf_sphere()
    host = r3d.TriangleMesh(vert, tri).compute_vertex_normals()
    dev = r3d.TriangleMesh(vert, tri).compute_vertex_normals(device=True)
    _bits(dev.vertex_normals, host.vertex_normals, "device against the numpy helper")
    n = dev.vertex_normals
    assert np.abs(np.sqrt((n * n).sum(1)) - 1.0).max() < 1e-15
    from tests import tsdf_mesh_cases as mc
    assert ((n * (vert - mc.SPHERE_C)).sum(1) > 0).all(), "a normal points inward"
    tn = r3d.TriangleMesh(vert, tri).compute_triangle_normals()
    assert tn.has_triangle_normals() and ((tn.triangle_normals * (vert[tri[:, 0]] - mc.SPHERE_C)).sum(1) > 0).all()
    # a zero-area triangle and a vertex without triangles: zero vectors stay zero
    vert, tri = tc.messy()
    iso = int(np.flatnonzero((vert == tc.MESSY_ISOLATED).all(1))[0])
    assert np.array_equal(r3d.mesh_ops.vertex_normals(vert, tri)[iso], np.zeros(3))
    flat = np.flatnonzero([len(set(r.tolist())) < 3 for r in tri])
    assert np.array_equal(r3d.mesh_ops.triangle_normals(vert, tri)[flat], np.zeros((1, 3)))


# ---- clean-ups -----------------------------------------------------------------------------------------------------------------------
def _dirty_grid():
    """the 70 x 70 grid with NaN and infinite vertices, degenerate triangles and vertices only those use"""
    vert, tri = tc.grid(70, 70)
    vert, tri = np.array(vert), np.array(tri)
    rng = np.random.default_rng(70)
    vert[rng.choice(len(vert), 40, replace=False), rng.integers(0, 3, 40)] = np.nan
    vert[rng.choice(len(vert), 10, replace=False), 0] = np.inf
    vert[rng.choice(len(vert), 5, replace=False), 2] = -np.inf
    rows = rng.choice(len(tri), 200, replace=False)
    tri[rows, 1] = tri[rows, rng.choice([0, 2], 200)]
    return vert, tri


def _check_compact(r3d, vert, tri, flags=0, vertex_keep=None, triangle_keep=None, what=""):
    nrm, col = tc.attributes(len(vert), 14)
    got = r3d.mesh_ops.compact(vert, tri, flags, vertex_keep, triangle_keep, nrm, col)
    want = tr.compact(vert, tri, flags, vertex_keep, triangle_keep, nrm, col)
    assert np.array_equal(np.isnan(got[0]), np.isnan(want[0]))
    for g, w, name in zip(got, want, ("vertices", "triangles", "normals", "colours")):
        _bits(np.nan_to_num(g, nan=0.0, posinf=1e300, neginf=-1e300), np.nan_to_num(w, nan=0.0, posinf=1e300, neginf=-1e300), f"{what} {name}")
    assert r3d.mesh_ops.compact_counts(vert, tri, flags, vertex_keep, triangle_keep) == (len(want[0]), len(want[1]))
    return got


@pytest.mark.parametrize("flags", (0, tr.DROP_DEGENERATE, tr.DROP_UNREFERENCED, tr.DROP_NON_FINITE, tr.DROP_DEGENERATE | tr.DROP_UNREFERENCED,
                                   tr.DROP_DEGENERATE | tr.DROP_UNREFERENCED | tr.DROP_NON_FINITE))
def test_compaction_flags(r3d, flags):
    for name, (vert, tri) in (("messy", tc.messy()), ("dirty grid", _dirty_grid()), ("fan300", tc.fan(300))):
        got = _check_compact(r3d, vert, tri, flags, what=f"{name} flags {flags}")
        if flags & tr.DROP_NON_FINITE:
            assert np.isfinite(got[0]).all()
        rng = np.random.default_rng(flags)
        _check_compact(r3d, vert, tri, flags, rng.random(len(vert)) < 0.9, rng.random(len(tri)) < 0.8, what=f"{name} flags {flags} with masks")
    vert, tri = _dirty_grid()
    kept = r3d.mesh_ops.compact(vert, tri, flags)
    if flags == 0:
        assert len(kept[0]) == len(vert) and len(kept[1]) == len(tri)
    if flags & tr.DROP_DEGENERATE:
        assert len(kept[1]) <= len(tri) - 200
    if flags & tr.DROP_NON_FINITE:
        assert len(kept[0]) < len(vert) and len(kept[1]) < len(tri)


def test_triangle_mesh_clean_ups(r3d):
    vert, tri = _dirty_grid()
    nrm, col = tc.attributes(len(vert), 15)

    def mesh():
        return r3d.TriangleMesh(vert, tri, col, nrm)

    def check(m, want):
        assert np.array_equal(m.vertices, want[0], equal_nan=True) and np.array_equal(m.triangles, want[1])
        _bits(m.vertex_normals, want[2])
        _bits(m.vertex_colors, want[3])

    m = mesh()
    assert m.remove_degenerate_triangles() is m
    check(m, tr.compact(vert, tri, tr.DROP_DEGENERATE, normals=nrm, colors=col))
    check(mesh().remove_unreferenced_vertices(), tr.compact(vert, tri, tr.DROP_UNREFERENCED, normals=nrm, colors=col))
    scrubbed = mesh().remove_non_finite_vertices()
    check(scrubbed, tr.compact(vert, tri, tr.DROP_NON_FINITE, normals=nrm, colors=col))
    assert np.isfinite(scrubbed.vertices).all() and len(scrubbed.vertices) == len(vert) - int((~np.isfinite(vert)).any(1).sum())
    check(mesh().remove_vertices_by_mask(~np.isfinite(vert).all(1)), tr.compact(vert, tri, tr.DROP_NON_FINITE, normals=nrm, colors=col))
    rng = np.random.default_rng(16)
    vm, tm = rng.random(len(vert)) < 0.2, rng.random(len(tri)) < 0.3
    check(mesh().remove_vertices_by_mask(vm), tr.compact(vert, tri, vertex_keep=~vm, normals=nrm, colors=col))
    check(mesh().remove_triangles_by_mask(tm), tr.compact(vert, tri, triangle_keep=~tm, normals=nrm, colors=col))
    # a mask that removes everything, and one that removes nothing
    gone = mesh().remove_vertices_by_mask(np.ones(len(vert), bool))
    assert gone.vertices.shape == (0, 3) and gone.triangles.shape == (0, 3) and gone.vertex_colors.shape == (0, 3) and not gone.has_vertices()
    same = mesh().remove_vertices_by_mask(np.zeros(len(vert), bool))
    assert np.array_equal(same.vertices, vert, equal_nan=True) and np.array_equal(same.triangles, tri)
    with pytest.raises(ValueError):
        mesh().remove_vertices_by_mask(np.ones(len(vert) - 1, bool))
    # triangle normals survive a clean-up that drops no triangle and are dropped by one that does
    tn = mesh().compute_triangle_normals()
    assert tn.remove_triangles_by_mask(np.zeros(len(tri), bool)).has_triangle_normals()
    assert tn.remove_degenerate_triangles().triangle_normals is None


def test_triangle_mesh_filters_and_lists(r3d):
    vert, tri = tc.noisy_sphere()
    nrm, col = tc.attributes(len(vert), 17)
    mesh = r3d.TriangleMesh(vert, tri, col, nrm)
    out = mesh.filter_smooth_laplacian(5)
    assert out is not mesh and np.array_equal(mesh.vertices, vert) and np.array_equal(out.triangles, tri)
    for g, w in zip((out.vertices, out.vertex_normals, out.vertex_colors), tr.smooth(tr.LAPLACIAN, vert, tri, 5, normals=nrm, colors=col)):
        _bits(g, w, "filter_smooth_laplacian(5)")
    v0, lap = tr.enclosed_volume(vert, tri), tr.enclosed_volume(out.vertices, tri)
    tau = tr.enclosed_volume(mesh.filter_smooth_taubin(5).vertices, tri)
    assert lap < v0 and abs(tau - v0) < abs(lap - v0)
    _bits(mesh.filter_smooth_simple(2, filter_scope=r3d.FilterScope.Vertex).vertices, tr.smooth(tr.SIMPLE, vert, tri, 2)[0], "filter_smooth_simple")
    _bits(mesh.filter_smooth_taubin(2, 0.4, -0.42, r3d.FilterScope.Color).vertex_colors,
          tr.smooth(tr.TAUBIN, vert, tri, 2, 0.4, -0.42, tr.COLOR, nrm, col)[2], "filter_smooth_taubin, colours")
    plain = r3d.TriangleMesh(vert, tri).filter_smooth_simple(1)
    assert plain.vertex_colors is None and plain.vertex_normals is None
    with pytest.raises(ValueError):
        mesh.filter_smooth_simple(-1)
    lists = mesh.compute_adjacency_list().adjacency_list
    assert mesh.has_adjacency_list() and [x.tolist() for x in lists] == tr.adjacency_literal(len(vert), tri)


# ---- interface -----------------------------------------------------------------------------------------------------------------------
def _compact_raw(ctx, vert, tri, flags, cap_v, cap_t, out_v, out_t, nrm=None, col=None, out_n=None, out_c=None):
    kv, kt = ctypes.c_int64(-5), ctypes.c_int64(-5)
    ctx.call("r3d_trimesh_compact", len(vert), len(tri), _p(vert), _p(nrm), _p(col), _p(tri), None, None, flags, cap_v, cap_t, _p(out_v), _p(out_n), _p(out_c),
             _p(out_t), ctypes.byref(kv), ctypes.byref(kt))
    return kv.value, kt.value


def test_capacities_repeats_and_resources(r3d, tmp_path):
    start = r3d._lib.live_resources()
    ctx = r3d.Context(0)                 # a context of its own: its arena goes with it
    mo = r3d.mesh_ops
    vert, tri = _dirty_grid()
    nrm, col = tc.attributes(len(vert), 18)
    flags = tr.DROP_DEGENERATE | tr.DROP_UNREFERENCED | tr.DROP_NON_FINITE
    want = tr.compact(vert, tri, flags, normals=nrm, colors=col)
    kv, kt = len(want[0]), len(want[1])
    assert 0 < kv < len(vert) and 0 < kt < len(tri)
    # a capacity one short on either side: R3D_E_BADARG, nothing written
    for cap_v, cap_t in ((kv - 1, kt), (kv, kt - 1), (kv, 0), (0, kt)):
        ov, on, oc, ot = np.full((kv, 3), 7.0), np.full((kv, 3), 7.0), np.full((kv, 3), 7.0), np.full((kt, 3), 7, np.int32)
        assert _code(_compact_raw, ctx, vert, tri, flags, cap_v, cap_t, ov, ot, nrm, col, on, oc) == -1
        assert (ov == 7.0).all() and (on == 7.0).all() and (oc == 7.0).all() and (ot == 7).all(), "a refused compaction wrote"
    # room to spare: the rows behind the result stay as they were
    ov, on, oc, ot = np.full((kv + 1, 3), 7.0), np.full((kv + 1, 3), 7.0), np.full((kv + 1, 3), 7.0), np.full((kt + 1, 3), 7, np.int32)
    assert _compact_raw(ctx, vert, tri, flags, kv + 1, kt + 1, ov, ot, nrm, col, on, oc) == (kv, kt)
    for g, w in zip((ov, ot, on, oc), want):
        _bits(g[:len(w)], w)
        assert (g[len(w):] == 7).all()
    assert _code(_compact_raw, ctx, vert, tri, flags, kv, kt, ov, ot, nrm, col, None, oc) == -1      # normals in, no room for them out
    assert _code(_compact_raw, ctx, vert, tri, flags, kv, kt, None, ot) == -1
    assert _code(_compact_raw, ctx, vert, tri, flags, kv, kt, ov, None) == -1
    assert _code(_compact_raw, ctx, vert, tri, flags, -1, kt, ov, ot) == -1
    assert _code(_compact_raw, ctx, vert, tri, 8, kv, kt, ov, ot) == -1                                # an unknown flag
    # adjacency with a capacity one short
    n = ctypes.c_int64()
    ctx.call("r3d_trimesh_adjacency", len(vert), len(tri), _p(tri), 0, None, None, ctypes.byref(n))
    want_off, want_nbs = tr.adjacency(len(vert), tri)
    assert n.value == len(want_nbs)
    off, lst = np.full(len(vert) + 1, 7, np.int32), np.full(n.value, 7, np.int32)
    assert _code(ctx.call, "r3d_trimesh_adjacency", len(vert), len(tri), _p(tri), n.value - 1, _p(off), _p(lst), ctypes.byref(n)) == -1
    assert (off == 7).all() and (lst == 7).all() and n.value == len(want_nbs)
    assert _code(ctx.call, "r3d_trimesh_adjacency", len(vert), len(tri), _p(tri), n.value, None, _p(lst), ctypes.byref(n)) == -1
    assert _code(ctx.call, "r3d_trimesh_incidence", len(vert), len(tri), _p(tri), 5, _p(off), _p(lst), None) == -1
    # two calls give identical bytes
    clean_v, clean_t = tc.tsdf_sphere()
    c_nrm, c_col = tc.attributes(len(clean_v), 19)
    for fn in (lambda: mo.adjacency(len(clean_v), clean_t, ctx=ctx), lambda: mo.incidence(len(clean_v), clean_t, ctx=ctx),
               lambda: mo.smooth(clean_v, clean_t, mo.SMOOTH_TAUBIN, 5, normals=c_nrm, colors=c_col, ctx=ctx),
               lambda: (mo.vertex_normals(clean_v, clean_t, ctx=ctx), mo.triangle_normals(clean_v, clean_t, ctx=ctx)),
               lambda: mo.compact(vert, tri, flags, normals=nrm, colors=col, ctx=ctx)):
        a, b = fn(), fn()
        assert [x.tobytes() for x in a] == [x.tobytes() for x in b]
    # the PLY round trip of a smoothed mesh
    smooth = r3d.TriangleMesh(clean_v, clean_t, c_col).filter_smooth_laplacian(5, ctx=ctx).compute_vertex_normals(device=True, ctx=ctx)
    path = str(tmp_path / "smooth.ply")
    r3d.io_formats.write_ply(path, smooth.vertices, normals=smooth.vertex_normals, colors=smooth.vertex_colors, faces=smooth.triangles)
    back = r3d.io_formats.read_ply(path)
    _bits(back["points"], smooth.vertices, "PLY vertices")
    _bits(back["normals"], smooth.vertex_normals, "PLY normals")
    assert np.array_equal(back["faces"], smooth.triangles)
    assert np.array_equal(back["colors"], np.floor(smooth.vertex_colors * 255 + 0.5).astype(np.uint8))
    held = r3d._lib.live_resources()
    assert held["device_allocs"] > start["device_allocs"]
    ctx.close()
    assert r3d._lib.live_resources() == start, "a triangle-mesh call left GPU resources behind"


def test_device_forms_with_sentinel_rows(r3d):
    ctx = r3d.Context(0)
    mo = r3d.mesh_ops
    vert, tri = tc.tsdf_sphere()
    nv, nt = len(vert), len(tri)
    nrm, col = tc.attributes(nv, 20)
    held = []

    def dev(a):
        held.append(ctx.to_device(a))
        return held[-1]

    def sentinel(rows, dtype=np.float64):
        return dev(np.full((rows + 1, 3), 7, dtype))

    def back(d, rows, dtype=np.float64):
        out = np.empty((rows + 1, 3), dtype)
        ctx.d2h(out, d)
        assert (out[rows:] == 7).all(), "a device form wrote behind its output"
        return out[:rows]

    try:
        d_v, d_n, d_c, d_t = dev(vert), dev(nrm), dev(col), dev(tri)
        for kind, n in ((tr.SIMPLE, 1), (tr.LAPLACIAN, 2), (tr.TAUBIN, 5), (tr.LAPLACIAN, 0)):
            o_v, o_n, o_c = sentinel(nv), sentinel(nv), sentinel(nv)
            mo.smooth_device(d_v, d_t, nv, nt, kind, n, o_v, d_normals=d_n, d_colors=d_c, d_out_normals=o_n, d_out_colors=o_c, ctx=ctx)
            for o, w in zip((o_v, o_n, o_c), tr.smooth(kind, vert, tri, n, normals=nrm, colors=col)):
                _bits(back(o, nv), w, f"smooth_dev kind {kind}, {n} iterations")
        o_v = sentinel(nv)
        mo.smooth_device(d_v, d_t, nv, nt, tr.LAPLACIAN, 3, o_v, scope=tr.VERTEX, ctx=ctx)       # no attributes at all
        _bits(back(o_v, nv), tr.smooth(tr.LAPLACIAN, vert, tri, 3)[0], "smooth_dev without attributes")
        check = np.empty_like(vert)                                                              # the inputs are untouched
        ctx.d2h(check, d_v)
        _bits(check, vert, "the input vertices")
        o_tn, o_vn = sentinel(nt), sentinel(nv)
        mo.normals_device(d_v, d_t, nv, nt, o_tn, o_vn, ctx=ctx)
        _bits(back(o_tn, nt), tr.triangle_normals(vert, tri), "normals_dev triangles")
        _bits(back(o_vn, nv), tr.vertex_normals(vert, tri), "normals_dev vertices")
        o_vn = sentinel(nv)
        mo.normals_device(d_v, d_t, nv, nt, None, o_vn, raw=True, ctx=ctx)
        _bits(back(o_vn, nv), tr.vertex_normals(vert, tri, raw=True), "normals_dev raw sums")
        # compaction on the device: drop a fifth of the vertices
        keep = (np.random.default_rng(21).random(nv) < 0.8).astype(np.uint8)
        want = tr.compact(vert, tri, tr.DROP_UNREFERENCED, vertex_keep=keep, normals=nrm, colors=col)
        kv, kt = len(want[0]), len(want[1])
        d_keep = dev(keep)
        o_v, o_n, o_c, o_t = sentinel(kv), sentinel(kv), sentinel(kv), sentinel(kt, np.int32)
        args = dict(d_vertex_keep=d_keep, d_normals=d_n, d_colors=d_c, d_out_normals=o_n, d_out_colors=o_c, ctx=ctx)
        assert mo.compact_device(d_v, d_t, nv, nt, tr.DROP_UNREFERENCED, 0, 0, None, None, d_vertex_keep=d_keep, ctx=ctx) == (kv, kt)
        assert _code(lambda: mo.compact_device(d_v, d_t, nv, nt, tr.DROP_UNREFERENCED, kv - 1, kt, o_v, o_t, **args)) == -1
        assert _code(lambda: mo.compact_device(d_v, d_t, nv, nt, tr.DROP_UNREFERENCED, kv, kt - 1, o_v, o_t, **args)) == -1
        for o, rows, dt in ((o_v, kv, np.float64), (o_n, kv, np.float64), (o_c, kv, np.float64), (o_t, kt, np.int32)):
            assert (back(o, rows, dt) == 7).all(), "a refused device compaction wrote"
        assert mo.compact_device(d_v, d_t, nv, nt, tr.DROP_UNREFERENCED, kv, kt, o_v, o_t, **args) == (kv, kt)
        for o, w, dt in ((o_v, want[0], np.float64), (o_t, want[1], np.int32), (o_n, want[2], np.float64), (o_c, want[3], np.float64)):
            _bits(back(o, len(w), dt), w, "compact_dev")
        # an output that is, or overlaps, an input or another output is refused before anything runs
        # (every array below is large enough for the call, should a refusal fail)
        big = max(nv, nt)
        spare, spare2, spare_t = sentinel(big), sentinel(big), sentinel(nt, np.int32)
        d_twice = dev(np.concatenate([vert, vert]))
        assert _code(lambda: mo.smooth_device(d_v, d_t, nv, nt, tr.LAPLACIAN, 1, d_v, ctx=ctx)) == -1
        assert _code(lambda: mo.smooth_device(d_twice, d_t, nv, nt, tr.LAPLACIAN, 0, d_twice + 24 * (nv - 1), ctx=ctx)) == -1      # one row shared
        assert _code(lambda: mo.smooth_device(d_v, d_t, nv, nt, tr.SIMPLE, 2, spare, d_normals=d_n, d_out_normals=d_c, d_colors=d_c, d_out_colors=spare2,
                                              ctx=ctx)) == -1
        assert _code(lambda: mo.smooth_device(d_v, d_t, nv, nt, tr.SIMPLE, 2, spare, d_normals=d_n, d_out_normals=spare, ctx=ctx)) == -1
        assert _code(lambda: mo.normals_device(d_v, d_t, nv, nt, None, d_v, ctx=ctx)) == -1
        assert _code(lambda: mo.normals_device(d_v, d_t, nv, nt, spare, spare, ctx=ctx)) == -1
        assert _code(lambda: mo.compact_device(d_v, d_t, nv, nt, 0, nv, nt, d_v, spare_t, ctx=ctx)) == -1
        assert _code(lambda: mo.compact_device(d_v, d_t, nv, nt, 0, nv, nt, spare, d_t, ctx=ctx)) == -1
        for host, d in ((vert, d_v), (nrm, d_n), (col, d_c), (tri, d_t)):
            check = np.empty_like(host)
            ctx.d2h(check, d)
            _bits(check, host, "an input after the refused calls")
        assert (back(spare, big) == 7).all() and (back(spare2, big) == 7).all() and (back(spare_t, nt, np.int32) == 7).all()
        mo.smooth_device(d_twice, d_t, nv, nt, tr.LAPLACIAN, 1, d_twice + 24 * nv, ctx=ctx)                # adjacent, not overlapping: accepted
    finally:
        for d in held:
            ctx.free(d)
        ctx.close()


def test_refusals(r3d):
    ctx = r3d.default_context()
    vert, tri = tc.noisy_sphere()
    vert, tri = np.array(vert), np.array(tri)
    nv, nt = len(vert), len(tri)
    out = np.full((nv, 3), 7.0)

    def smooth(nv_=nv, nt_=nt, v=vert, t=tri, kind=tr.LAPLACIAN, n=1, lam=0.5, mu=-0.53, scope=tr.ALL, o=out, nrm=None, o_n=None):
        ctx.call("r3d_trimesh_smooth", nv_, nt_, _p(v), _p(nrm), None, _p(t), kind, n, lam, mu, scope, _p(o), _p(o_n), None)

    smooth()                                                                                    # the arguments below differ from a good call in one thing
    assert not (out == 7.0).any()
    out[:] = 7.0
    for kw in (dict(v=None), dict(t=None), dict(o=None), dict(nrm=vert), dict(nv_=-1), dict(nt_=-1), dict(n=-1), dict(lam=np.nan), dict(lam=np.inf),
               dict(mu=-np.inf), dict(mu=np.nan), dict(kind=3), dict(kind=-1), dict(scope=4), dict(scope=-1)):
        assert _code(lambda: smooth(**kw)) == -1, kw
    assert _code(lambda: smooth(nt_=(1 << 31) // 6 + 1)) == -4 and _code(lambda: smooth(nv_=(1 << 31) - 1)) == -4
    assert _code(lambda: smooth(n=(1 << 20) + 1)) == -4 and _code(lambda: smooth(n=(1 << 31) - 1, kind=tr.TAUBIN)) == -4    # a launch per step
    assert (out == 7.0).all(), "a refused call wrote"
    # an index outside [0, nv): as the last corner of the last triangle, and as -1; every entry point, nothing written
    for bad in (nv, -1, 1 << 30, -(1 << 31)):
        t = tri.copy()
        t[-1, 2] = bad
        assert _code(lambda: smooth(t=t)) == -1
        assert _code(lambda: smooth(t=t, n=0)) == -1
        assert (out == 7.0).all(), "a refused call wrote"
        n = ctypes.c_int64()
        for entry in ("r3d_trimesh_incidence", "r3d_trimesh_adjacency"):
            assert _code(ctx.call, entry, nv, nt, _p(t), 0, None, None, ctypes.byref(n)) == -1
        assert _code(ctx.call, "r3d_trimesh_normals", nv, nt, _p(vert), _p(t), 0, _p(out), None) == -1
        assert _code(ctx.call, "r3d_trimesh_normals", nv, nt, _p(vert), _p(t), 0, None, _p(out)) == -1
        assert _code(_compact_raw, ctx, vert, t, 0, 0, 0, None, None) == -1
        assert _code(_compact_raw, ctx, vert, t, tr.DROP_UNREFERENCED, nv, nt, out, np.empty((nt, 3), np.int32)) == -1
        assert (out == 7.0).all(), "a refused call wrote"
    first = tri.copy()
    first[0, 0] = nv
    assert _code(lambda: smooth(t=first)) == -1
    assert _code(ctx.call, "r3d_trimesh_normals", nv, nt, _p(vert), _p(tri), 2, _p(out), None) == -1          # unknown flags
    assert _code(ctx.call, "r3d_trimesh_normals", nv, nt, None, _p(tri), 0, _p(out), None) == -1
    assert _code(ctx.call, "r3d_trimesh_normals", nv, nt, _p(vert), None, 0, _p(out), None) == -1
    assert _code(ctx.call, "r3d_trimesh_normals", -1, nt, _p(vert), _p(tri), 0, _p(out), None) == -1
    assert _code(lambda: smooth(nv_=0)) == -1                                                    # triangles without vertices
    # the context still works
    _bits(r3d.mesh_ops.smooth(vert, tri, tr.LAPLACIAN, 1)[0], tr.smooth(tr.LAPLACIAN, vert, tri, 1)[0])


def test_empty_meshes(r3d):
    mo = r3d.mesh_ops
    none_v, none_t = np.zeros((0, 3)), np.zeros((0, 3), np.int32)
    off, lst = mo.adjacency(0, none_t)
    assert off.tolist() == [0] and lst.shape == (0,)
    assert mo.incidence(0, none_t)[0].tolist() == [0]
    assert [None if a is None else a.shape for a in mo.smooth(none_v, none_t, tr.TAUBIN, 3)] == [(0, 3), None, None]
    assert mo.vertex_normals(none_v, none_t).shape == (0, 3) and mo.triangle_normals(none_v, none_t).shape == (0, 3)
    assert [None if a is None else a.shape for a in mo.compact(none_v, none_t, 7)] == [(0, 3), (0, 3), None, None]
    empty = r3d.TriangleMesh()
    assert empty.filter_smooth_laplacian(5).vertices.shape == (0, 3) and empty.remove_non_finite_vertices() is empty
    assert empty.compute_vertex_normals(device=True).vertex_normals.shape == (0, 3) and empty.compute_adjacency_list().adjacency_list == []
    # vertices without triangles: empty lists, copies and zero normals
    vert = np.array(tc.noisy_sphere()[0])
    nrm, col = tc.attributes(len(vert), 22)
    off, lst = mo.adjacency(len(vert), none_t)
    assert not off.any() and len(off) == len(vert) + 1 and lst.shape == (0,)
    assert not mo.incidence(len(vert), none_t)[0].any()
    for kind in KINDS:
        for g, w in zip(mo.smooth(vert, none_t, kind, 3, normals=nrm, colors=col), (vert, nrm, col)):
            _bits(g, w, "no triangles")
    assert not mo.vertex_normals(vert, none_t).any()
    kept = mo.compact(vert, none_t, tr.DROP_DEGENERATE | tr.DROP_NON_FINITE, colors=col)
    _bits(kept[0], vert)
    _bits(kept[3], col)
    assert kept[1].shape == (0, 3) and mo.compact(vert, none_t, tr.DROP_UNREFERENCED)[0].shape == (0, 3)


def test_tsdf_fuse_with_postprocess(r3d):
    """tsdf_fuse(mesh=True, postprocess=True) on case A of the volume tests equals the steps done by hand"""
    from tests import rgbd_scene as sc
    from tests import test_tsdf_gpu as tg
    frames = []
    for k in range(3):
        depth, color = tg._frame(64, 48, k)
        frames.append((color, np.round(depth * 1000.0).astype(np.uint16)))
    cam = sc.camera(64, 48)
    camera = r3d.cloud_ops.depth_camera(dict(fx=cam[0], fy=cam[1], ppx=cam[2], ppy=cam[3]), depth_scale=1000.0, depth_trunc=3.0)
    raw = r3d.pipeline.tsdf_fuse(frames, camera, list(tg.POSES_A), tg.VL, tg.TRUNC, color=True, initial_units=8, mesh=True)
    done = r3d.pipeline.tsdf_fuse(frames, camera, list(tg.POSES_A), tg.VL, tg.TRUNC, color=True, initial_units=8, mesh=True, postprocess=True)
    assert raw.has_triangles() and raw.vertex_normals is None and done.has_vertex_normals() and done.has_vertex_colors()
    # by hand, with the restatement
    pos, _, col = tr.smooth(tr.LAPLACIAN, raw.vertices, raw.triangles, 5, colors=raw.vertex_colors)
    v, t, _, c = tr.compact(pos, raw.triangles, tr.DROP_DEGENERATE, colors=col)
    v, t, _, c = tr.compact(v, t, tr.DROP_NON_FINITE, colors=c)
    v, t, _, c = tr.compact(v, t, tr.DROP_UNREFERENCED, colors=c)
    _bits(done.vertices, v, "post-processed vertices")
    _bits(done.vertex_colors, c, "post-processed colours")
    _bits(done.triangles, t, "post-processed triangles")
    _bits(done.vertex_normals, tr.vertex_normals(v, t), "post-processed normals")
    # and with the mesh's own methods
    hand = raw.filter_smooth_laplacian(5).remove_degenerate_triangles().remove_non_finite_vertices().remove_unreferenced_vertices()
    hand.compute_vertex_normals()
    assert np.isfinite(done.vertices).all()
    _bits(hand.vertices, done.vertices)
    _bits(hand.triangles, done.triangles)
    _bits(hand.vertex_normals, done.vertex_normals)
    again = r3d.pipeline.mesh_postprocess(raw)
    assert again.vertices.tobytes() == done.vertices.tobytes() and again.vertex_normals.tobytes() == done.vertex_normals.tobytes()
    with pytest.raises(ValueError):
        r3d.pipeline.tsdf_fuse(frames, camera, list(tg.POSES_A), tg.VL, tg.TRUNC, postprocess=True)
