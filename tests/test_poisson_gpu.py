"""GPU tests of the Poisson reconstruction ("Poisson reconstruction"): the fields and chi of
r3d_debug_poisson_fields, the marching cubes of r3d_debug_poisson_extract and the whole reconstruction, each bit for bit against
tests/poisson_ref.py; the capacity protocol, the refusals and the resources.  Everything stays at depth <= 6."""
import ctypes
import os

import numpy as np
import pytest

from tests import poisson_ref as ref
from tests import trimesh_ref as tr
from tests.conftest import GOLDEN
from tests.tsdf_mesh_ref import CORNERS, edge_census, signed_volume

pytestmark = pytest.mark.gpu

FIELDS = ("W0", "C0", "dens", "V", "D", "b")


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _bits(got, want, what=""):
    if want is None:
        assert got is None, what
        return
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if got.tobytes() != want.tobytes():
        bad = np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))
        raise AssertionError(f"{what}: {len(bad)} of {got.size} entries differ, first at {bad[0] if len(bad) else '(sign of zero)'}")


def _code(r3d, fn, *args, **kw):
    with pytest.raises(r3d.R3DError) as e:
        fn(*args, **kw)
    return e.value.code


@pytest.fixture(scope="module")
def table(r3d):
    return r3d.tsdf.mc_table()


# ---- fields and chi --------------------------------------------------------------------------------------------------------------------
def _check_fields(r3d, pts, nrm, col, **prm):
    """W0, C0, dens, V, D, b, and chi after the first and after the last cycle"""
    p = ref.params(**prm)
    history = []
    want = ref.fields(pts, nrm, col, p, history=history)
    dp = r3d.poisson.poisson_params(**prm)
    first = r3d.poisson.debug_fields(pts, nrm, col, dp, k_cycles=1)
    last = r3d.poisson.debug_fields(pts, nrm, col, dp)
    assert first["G"] == want["G"]
    for got in (first, last):
        _bits(got["org"], want["org"], "org")
        assert got["h"] == want["h"]
        for name in FIELDS:
            _bits(got[name], want[name], name)
    _bits(first["chi"], history[0], "chi after cycle 1")
    _bits(last["chi"], history[-1], "chi after the last cycle")
    assert np.abs(history[-1]).max() > 0 or not np.asarray(nrm).any()
    return want


def _noisy_sphere(n, seed, hemisphere=False):
    return ref.sphere_cloud(n, 0.7, noise=0.01, seed=seed, hemisphere=hemisphere)


def test_depth_2_runs_the_coarsest_sweeps_only(r3d):
    _check_fields(r3d, *_noisy_sphere(300, 2), depth=2)


def test_depth_3_coarsens_once(r3d):
    _check_fields(r3d, *_noisy_sphere(300, 3), depth=3)


@pytest.mark.parametrize("depth", [4, 5])
@pytest.mark.parametrize("hemisphere", [False, True], ids=["sphere", "hemisphere"])
def test_noisy_sphere_and_open_hemisphere(r3d, depth, hemisphere):
    _check_fields(r3d, *_noisy_sphere(2000, 10 * depth + hemisphere, hemisphere), depth=depth)


def test_hand_placed_points(r3d):
    """depth 5, scale 1: the cloud's box is the grid, h = 1/32.  Points on grid nodes, on cell faces, on the cube's faces (f = 1 in
    the last cell), the same point twice, and two zero-length normals"""
    h = 1.0 / 32
    pts = np.array([[0.0, 0.0, 0.0], [1.0, 1.0, 1.0],                       # the box's corners: node 0 and the top node
                    [0.5, 0.5, 0.5], [8 * h, 20 * h, 3 * h],                # interior nodes
                    [5 * h, 0.3011, 0.7713], [0.4142, 17 * h, 0.2718],      # on a cell face
                    [1.0, 0.3, 0.7], [0.25, 1.0, 0.6], [0.66, 0.41, 1.0],   # on the cube's top faces
                    [0.1234, 0.0, 0.9],                                     # on a bottom face
                    [0.37, 0.59, 0.83], [0.37, 0.59, 0.83]])                # twice
    rng = np.random.default_rng(5)
    nrm = rng.standard_normal((12, 3))
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    nrm[3] = 0.0
    nrm[10] = 0.0
    want = _check_fields(r3d, pts, nrm, rng.random((12, 3)), depth=5, scale=1.0)
    assert want["h"] == h and (want["org"] == 0.0).all()
    cell, f = ref.cells(pts, want["org"], want["h"], 32)
    assert (cell[1] == 31).all() and (f[1] == 1.0).all() and (f[0] == 0.0).all() and f[6, 0] == 1.0 and f[7, 1] == 1.0 and f[8, 2] == 1.0


def test_one_crowded_cell(r3d):
    """700 points in one cell, more than any workgroup has threads, beside empty cells and a few lone points"""
    rng = np.random.default_rng(6)
    lone = rng.uniform(-1.0, 1.0, (40, 3))
    lone[0], lone[1] = [-1.0, -1.0, -1.0], [1.0, 1.0, 1.0]
    h = 2.2 / 32
    corner = np.floor((np.array([0.31, -0.17, 0.55]) + 1.1) / h) * h - 1.1
    crowd = corner + h * rng.uniform(0.05, 0.95, (700, 3))
    pts = np.concatenate([lone[:20], crowd, lone[20:]])
    nrm = rng.standard_normal((len(pts), 3))
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    want = _check_fields(r3d, pts, nrm, rng.random((len(pts), 3)), depth=5)
    cell, _ = ref.cells(pts, want["org"], want["h"], 32)
    assert (np.unique(cell, axis=0, return_counts=True)[1] >= 700).sum() == 1


def test_flat_cloud(r3d):
    """every point in the plane z = 0.25"""
    rng = np.random.default_rng(7)
    pts = np.concatenate([rng.uniform(-0.5, 0.5, (1500, 2)), np.full((1500, 1), 0.25)], 1)
    nrm = np.tile([0.0, 0.0, 1.0], (1500, 1))
    _check_fields(r3d, pts, nrm, None, depth=5)


def test_zero_length_normals_are_accepted(r3d):
    pts, _, col = _noisy_sphere(500, 8)
    want = _check_fields(r3d, pts, np.zeros_like(pts), col, depth=4, cycles=2)
    assert not want["chi"].any() and not want["b"].any() and want["D"].any()


# ---- extraction ------------------------------------------------------------------------------------------------------------------------
def _check_extract(r3d, table, chi, W0, C0, org, h):
    want = ref.extract(chi, W0, C0, org, h, table)
    got = r3d.poisson.debug_extract(chi, W0, C0, org, h)
    for g, w, name in zip(got, want, ("vertices", "densities", "colours", "triangles")):
        _bits(g, w, name)
    vert, _, _, tri = got
    if len(tri):
        assert tri.min() >= 0 and tri.max() < len(vert), "an index outside [0, nv)"
        assert len(np.unique(tri)) == len(vert), "a vertex no triangle uses"
    return got


def _attributes(G, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(0.5, 3.0, (G, G, G)), rng.uniform(0.0, 2.0, (3, G, G, G))


def test_all_256_cube_configurations(r3d, table):
    """a 2x2x2 block of nodes per configuration on a pitch of 3 nodes in a 33^3 grid; everything else is outside"""
    G = 33
    rng = np.random.default_rng(9)
    chi = rng.uniform(0.5, 1.5, (G, G, G))
    for c in range(256):
        bx, by, bz = 1 + 3 * (c % 7), 1 + 3 * ((c // 7) % 7), 1 + 3 * (c // 49)
        for bit, (ox, oy, oz) in enumerate(CORNERS):
            if (c >> bit) & 1:
                chi[bz + oz, by + oy, bx + ox] = -rng.uniform(0.5, 1.5)
    W0, C0 = _attributes(G, 10)
    vert, _, _, tri = _check_extract(r3d, table, chi, W0, C0, np.array([-1.0, 0.5, 2.0]), 0.125)
    count = (np.asarray(table).reshape(256, 16) >= 0).sum(1) // 3
    inside = chi < 0
    cube = np.zeros((G - 1, G - 1, G - 1), np.int64)
    for bit, (ox, oy, oz) in enumerate(CORNERS):
        cube |= inside[oz:oz + G - 1, oy:oy + G - 1, ox:ox + G - 1].astype(np.int64) << bit
    for c in range(256):
        assert cube[1 + 3 * (c // 49), 1 + 3 * ((c // 7) % 7), 1 + 3 * (c % 7)] == c
    # triangles come cube by cube: every cube contributes its row's count
    starts = np.concatenate([[0], np.cumsum(count[cube.reshape(-1)])])
    assert len(tri) == starts[-1]
    repeated, boundary, _ = edge_census(tri)
    assert repeated == 0 and boundary == 0


def test_zero_and_negative_zero_are_outside_and_t_reaches_one(r3d, table):
    G = 5
    chi = np.full((G, G, G), 1.0)
    chi[2, 2, 2] = -1.0
    chi[2, 2, 3] = 0.0             # chi_b = 0 behind chi_a < 0: t = 1
    chi[2, 3, 2] = -0.0            # outside as well
    chi[1, 2, 2] = 0.0             # chi_a = 0 before chi_b < 0: t = 0
    chi[2, 2, 1] = -0.0
    W0, C0 = _attributes(G, 11)
    W0[2, 2, 3] = 0.0              # a zero density at a vertex: a zero colour
    org, h = np.array([0.0, 0.0, 0.0]), 0.5
    vert, dens, col, tri = _check_extract(r3d, table, chi, W0, C0, org, h)
    assert len(vert) == 6 and len(tri) == 8
    nodes = {tuple(v) for v in vert / h}
    assert {(3.0, 2.0, 2.0), (2.0, 3.0, 2.0), (2.0, 2.0, 1.0), (1.0, 2.0, 2.0)} <= nodes
    at = [tuple(v) for v in vert / h].index((3.0, 2.0, 2.0))
    assert dens[at] == 0.0 and (col[at] == 0.0).all()


def test_slanted_plane_on_65_cubed(r3d, table):
    """several workgroups per axis and the carry of the offsets through the scan's tiles"""
    G = 65
    k, j, i = np.meshgrid(np.arange(G), np.arange(G), np.arange(G), indexing="ij")
    chi = (0.37 * i + 0.23 * j + 0.61 * k - 30.3) / 7.0
    chi[[0, -1]] = chi[:, [0, -1]] = chi[:, :, [0, -1]] = 0.0
    W0, C0 = _attributes(G, 12)
    vert, _, _, tri = _check_extract(r3d, table, chi, W0, C0, np.array([0.1, -0.2, 0.3]), 0.03)
    assert len(vert) > 8192 and len(tri) > 8192
    assert edge_census(tri)[:2] == (0, 0)


def test_extract_without_colours(r3d, table):
    G = 17
    rng = np.random.default_rng(13)
    chi = rng.standard_normal((G, G, G))
    chi[[0, -1]] = chi[:, [0, -1]] = chi[:, :, [0, -1]] = 0.0
    W0, _ = _attributes(G, 14)
    got = _check_extract(r3d, table, chi, W0, None, np.zeros(3), 1.0)
    assert got[2] is None and len(got[3]) > 0


def _extract_raw(ctx, depth, org, h, chi, W0, C0, cap_v, cap_t, vert, dens, col, tri):
    nv, nt = ctypes.c_int64(-5), ctypes.c_int64(-5)
    rc = ctx._lib.r3d_debug_poisson_extract(ctx._h, depth, _p(org), h, _p(chi), _p(W0), _p(C0), cap_v, cap_t, _p(vert), _p(dens), _p(col), _p(tri),
                                            ctypes.byref(nv), ctypes.byref(nt))
    return rc, nv.value, nt.value


def test_counts_alone_and_capacities_one_short(r3d, table):
    ctx = r3d.default_context()
    G = 9
    rng = np.random.default_rng(15)
    chi = rng.standard_normal((G, G, G))
    chi[[0, -1]] = chi[:, [0, -1]] = chi[:, :, [0, -1]] = 0.0
    W0, C0 = _attributes(G, 16)
    org = np.zeros(3)
    want = ref.extract(chi, W0, C0, org, 1.0, table)
    nv, nt = len(want[0]), len(want[3])
    assert nv > 0 and nt > 0
    assert _extract_raw(ctx, 3, org, 1.0, chi, W0, C0, 0, 0, None, None, None, None) == (0, nv, nt)
    for cap_v, cap_t in ((nv - 1, nt), (nv, nt - 1), (nv, 0), (0, nt)):
        vert, dens, col, tri = np.full((nv, 3), 7.0), np.full(nv, 7.0), np.full((nv, 3), 7.0), np.full((nt, 3), 7, np.int32)
        assert _extract_raw(ctx, 3, org, 1.0, chi, W0, C0, cap_v, cap_t, vert, dens, col, tri) == (-1, nv, nt)
        assert (vert == 7.0).all() and (dens == 7.0).all() and (col == 7.0).all() and (tri == 7).all(), "a refused extraction wrote"
    # room to spare: the rows behind the result stay as they were
    vert, dens, col, tri = np.full((nv + 1, 3), 7.0), np.full(nv + 1, 7.0), np.full((nv + 1, 3), 7.0), np.full((nt + 1, 3), 7, np.int32)
    assert _extract_raw(ctx, 3, org, 1.0, chi, W0, C0, nv + 1, nt + 1, vert, dens, col, tri) == (0, nv, nt)
    for g, w in zip((vert, dens, col, tri), want):
        _bits(g[:len(w)], w)
        assert (g[len(w):] == 7).all()
    # a missing array, a negative capacity, a depth the grid does not have
    assert _extract_raw(ctx, 3, org, 1.0, chi, W0, C0, nv, nt, vert, None, col, tri)[0] == -1
    assert _extract_raw(ctx, 3, org, 1.0, chi, W0, C0, nv, nt, vert, dens, None, tri)[0] == -1
    assert _extract_raw(ctx, 3, org, 1.0, chi, W0, C0, nv, -1, vert, dens, col, tri)[0] == -1
    assert _extract_raw(ctx, 9, org, 1.0, chi, W0, C0, nv, nt, vert, dens, col, tri)[0] == -4


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def spheres():
    """lattice spheres that sample every surface cell: 4 000 points for depth 5 (h = 0.048), 12 000 for depth 6 (h = 0.024)"""
    return {5: ref.sphere_cloud(4000, 0.7, noise=0.003, seed=21, lattice=True), 6: ref.sphere_cloud(12000, 0.7, noise=0.0015, seed=22, lattice=True)}


@pytest.mark.parametrize("depth", [5, 6])
def test_sphere_equals_the_restatement(r3d, table, spheres, depth):
    pts, nrm, col = spheres[depth]
    want = ref.reconstruct(pts, nrm, col, ref.params(depth=depth), table)
    mesh, dens = r3d.create_from_point_cloud_poisson(r3d.PointCloud(pts, col, nrm), depth=depth)
    _bits(mesh.vertices, want[0], "vertices")
    _bits(dens, want[1], "densities")
    _bits(mesh.vertex_colors, want[2], "colours")
    _bits(mesh.triangles, want[3], "triangles")
    nv, nt = len(mesh.vertices), len(mesh.triangles)
    assert dens.shape == (nv,) and nt > 0
    repeated, boundary, undirected = edge_census(mesh.triangles)
    assert repeated == 0 and boundary == 0, "the mesh is not closed"
    assert nv - undirected + nt == 2
    assert signed_volume(mesh.vertices, mesh.triangles) > 0
    mesh.compute_vertex_normals(device=True)
    assert ((mesh.vertex_normals * mesh.vertices).sum(1) > 0).all(), "a vertex normal looks inward"
    # the second call, and the method form, give identical bytes
    again, dens2 = r3d.TriangleMesh.create_from_point_cloud_poisson(r3d.PointCloud(pts, col, nrm), depth=depth)
    assert (again.vertices.tobytes(), again.triangles.tobytes(), again.vertex_colors.tobytes(), dens2.tobytes()) == \
        (mesh.vertices.tobytes(), mesh.triangles.tobytes(), mesh.vertex_colors.tobytes(), dens.tobytes())
    # trimming by density, as Open3D's users do
    low = dens < np.quantile(dens, 0.1)
    assert 0 < low.sum() < nv
    trimmed = r3d.TriangleMesh(mesh.vertices, mesh.triangles, mesh.vertex_colors).remove_vertices_by_mask(low)
    assert len(trimmed.vertices) == nv - low.sum() and 0 < len(trimmed.triangles) < nt


def test_golden_frame_through_the_stage_class(r3d, table):
    """tests/golden/output/pcd_00008.ply with its recorded normals: MeshReconstruction().reconstruct_mesh equals the restatement's
    Poisson at depth 6 followed by the restated mesh chain"""
    ply = r3d.io_formats.read_ply(os.path.join(GOLDEN, "output", "pcd_00008.ply"))
    cloud = r3d.PointCloud(ply["points"], ply.get("colors_f"), ply["normals"])
    assert cloud.has_normals()
    col = cloud.colors if cloud.has_colors() else None
    done = r3d.MeshReconstruction().reconstruct_mesh(cloud)
    vert, _, vcol, tri = ref.reconstruct(cloud.points, cloud.normals, col, ref.params(depth=6), table)
    assert len(tri) > 0
    pos, _, c = tr.smooth(tr.LAPLACIAN, vert, tri, 5, colors=vcol)
    v, t, _, c = tr.compact(pos, tri, tr.DROP_DEGENERATE, colors=c)
    v, t, _, c = tr.compact(v, t, tr.DROP_NON_FINITE, colors=c)
    v, t, _, c = tr.compact(v, t, tr.DROP_UNREFERENCED, colors=c)
    _bits(done.vertices, v, "vertices")
    _bits(done.triangles, t, "triangles")
    if col is not None:
        _bits(done.vertex_colors, c, "colours")
    _bits(done.vertex_normals, tr.vertex_normals(v, t), "normals")
    again = r3d.pipeline.reconstruct_mesh(cloud)
    assert again.vertices.tobytes() == done.vertices.tobytes() and again.triangles.tobytes() == done.triangles.tobytes()


def _reconstruct_raw(ctx, r3d, pts, nrm, col, prm, cap_v, cap_t, out, dev=False):
    nv, nt = ctypes.c_int64(-5), ctypes.c_int64(-5)
    fn = ctx._lib.r3d_poisson_reconstruct_dev if dev else ctx._lib.r3d_poisson_reconstruct
    as_arg = (lambda a: ctypes.c_void_p(a)) if dev else _p
    rc = fn(ctx._h, as_arg(pts), as_arg(nrm), as_arg(col), (len(pts) if not dev else out["n"]), ctypes.byref(prm), cap_v, cap_t, as_arg(out["vert"]),
            as_arg(out["dens"]), as_arg(out["col"]), as_arg(out["tri"]), ctypes.byref(nv), ctypes.byref(nt))
    return rc, nv.value, nt.value


def test_refusals_write_nothing(r3d):
    ctx = r3d.default_context()
    pts, nrm, col = ref.sphere_cloud(500, 0.7, seed=30)
    P = r3d.poisson.poisson_params

    def refused(pts, nrm, col, prm, code):
        out = dict(vert=np.full((64, 3), 7.0), dens=np.full(64, 7.0), col=np.full((64, 3), 7.0), tri=np.full((64, 3), 7, np.int32))
        rc, nv, nt = _reconstruct_raw(ctx, r3d, pts, nrm, col, prm, 64, 64, out)
        assert rc == code, (rc, code, ctx._lib.r3d_last_error(ctx._h))
        assert all((a == 7).all() for a in out.values()), "a refused reconstruction wrote"

    refused(pts, None, col, P(depth=4), -1)                                   # no normals
    refused(pts[:0], nrm[:0], None, P(depth=4), -1)                           # n = 0
    refused(np.tile(pts[:1], (50, 1)), nrm[:50], None, P(depth=4), -1)         # identical points: s = 0
    bad = pts.copy()
    bad[123, 1] = np.nan
    refused(bad, nrm, col, P(depth=4), -1)
    bad = nrm.copy()
    bad[7, 2] = np.inf
    refused(pts, bad, col, P(depth=4), -1)
    refused(pts, nrm, col, P(depth=1), -4)
    refused(pts, nrm, col, P(depth=9), -4)
    refused(pts, nrm, col, P(depth=4, cycles=-1), -1)
    cloud = r3d.PointCloud(pts, col, nrm)
    assert _code(r3d, r3d.create_from_point_cloud_poisson, cloud, depth=4, linear_fit=True) == -4
    assert _code(r3d, r3d.create_from_point_cloud_poisson, cloud, depth=4, width=1) == -4
    assert _code(r3d, r3d.create_from_point_cloud_poisson, r3d.PointCloud(pts, col), depth=4) == -1
    assert _code(r3d, r3d.create_from_point_cloud_poisson, cloud, depth=9) == -4
    assert _code(r3d, r3d.poisson.debug_fields, pts, nrm, None, P(depth=4), 11) == -1          # k_cycles > cycles
    # and the context still works
    mesh, dens = r3d.create_from_point_cloud_poisson(cloud, depth=4)
    assert mesh.has_triangles() and len(dens) == len(mesh.vertices)


def test_device_form_counts_capacities_and_resources(r3d, table):
    start = r3d._lib.live_resources()
    ctx = r3d.Context(0)                 # a context of its own: its arena goes with it
    pts, nrm, col = ref.sphere_cloud(1500, 0.7, noise=0.005, seed=31, lattice=True)
    prm = r3d.poisson.poisson_params(depth=4)
    want = r3d.poisson.reconstruct(pts, nrm, col, prm, ctx=ctx)
    for w, r in zip(want, ref.reconstruct(pts, nrm, col, ref.params(depth=4), table)):
        _bits(w, r)
    nv, nt = len(want[0]), len(want[3])
    host = dict(vert=None, dens=None, col=None, tri=None)
    assert _reconstruct_raw(ctx, r3d, pts, nrm, col, prm, 0, 0, host) == (0, nv, nt)                 # the counts alone
    for cap_v, cap_t in ((nv - 1, nt), (nv, nt - 1)):
        out = dict(vert=np.full((nv, 3), 7.0), dens=np.full(nv, 7.0), col=np.full((nv, 3), 7.0), tri=np.full((nt, 3), 7, np.int32))
        assert _reconstruct_raw(ctx, r3d, pts, nrm, col, prm, cap_v, cap_t, out) == (-1, nv, nt)
        assert all((a == 7).all() for a in out.values())
    # the device form, a sentinel row behind each output
    sent = dict(vert=np.full((nv + 1, 3), 7.0), dens=np.full(nv + 1, 7.0), col=np.full((nv + 1, 3), 7.0), tri=np.full((nt + 1, 3), 7, np.int32))
    d_in = [ctx.to_device(a) for a in (pts, nrm, col)]
    d_out = {k: ctx.to_device(a) for k, a in sent.items()}
    d_out["n"] = len(pts)
    try:
        assert _reconstruct_raw(ctx, r3d, d_in[0], d_in[1], d_in[2], prm, nv, nt, d_out, dev=True) == (0, nv, nt)
        assert _reconstruct_raw(ctx, r3d, d_in[0], d_in[1], d_in[2], prm, 0, 0, d_out, dev=True) == (0, nv, nt)
        assert _reconstruct_raw(ctx, r3d, d_in[0], d_in[1], d_in[2], prm, nv, nt - 1, d_out, dev=True) == (-1, nv, nt)
        for k, w in zip(("vert", "dens", "col", "tri"), want):
            got = np.empty_like(sent[k])
            ctx.d2h(got, d_out[k])
            _bits(got[:len(w)], w, k)
            assert (got[len(w):] == 7).all(), f"{k}: the row behind the result changed"
    finally:
        for ptr in d_in + [d_out[k] for k in sent]:
            ctx.free(ptr)
    held = r3d._lib.live_resources()
    assert held["device_allocs"] > start["device_allocs"]
    ctx.close()
    assert r3d._lib.live_resources() == start, "a Poisson reconstruction left GPU resources behind"
