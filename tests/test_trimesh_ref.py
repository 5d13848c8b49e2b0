"""CPU tests of the triangle-mesh contract's restatement (tests/trimesh_ref.py): its literal and its vectorised form agree bit for
bit, and the filters behave as filters ("Triangle-mesh operations")."""
import numpy as np
import pytest

from tests import trimesh_cases as tc
from tests import trimesh_ref as tr

BIG = 2000      # vertices from which the literal filters run one iteration instead of two


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint64) if a.dtype == np.float64 else a,
                                                                        b.view(np.uint64) if b.dtype == np.float64 else b)


@pytest.mark.parametrize("name", sorted(tc.CASES))
def test_lists_literal_equals_vectorised_and_sets(name):
    vert, tri = tc.CASES[name]()
    nv = len(vert)
    off, corners = tr.incidence(nv, tri)
    assert tr.csr_to_lists(off, corners) == tr.incidence_literal(nv, tri)
    assert all(tri.reshape(-1)[c] == v for v in range(nv) for c in corners[off[v]:off[v + 1]])
    aoff, nbs = tr.adjacency(nv, tri)
    lists = tr.csr_to_lists(aoff, nbs)
    assert lists == tr.adjacency_literal(nv, tri)
    # a set-based construction written another way: the vertices of the triangles at v, without the corner that is v itself
    flat = tri.reshape(-1)
    for v in range(nv):
        want = set()
        for c in corners[off[v]:off[v + 1]]:
            t = c // 3
            want.update(int(flat[3 * t + k]) for k in range(3) if 3 * t + k != c)
        assert set(lists[v]) == want and lists[v] == sorted(want)


def test_lists_of_the_big_grid_vectorised_only():
    vert, tri = tc.big_grid()
    nv = len(vert)
    assert nv == 1025 * 1025 and len(tri) == 2 * 1024 * 1024
    off, corners = tr.incidence(nv, tri)
    assert off[-1] == 3 * len(tri) and np.array_equal(tri.reshape(-1)[corners], np.repeat(np.arange(nv), np.diff(off)))
    aoff, nbs = tr.adjacency(nv, tri)
    deg = np.diff(aoff)
    assert deg.min() == 2 and deg.max() == 6 and int((deg == 6).sum()) == 1023 * 1023


def test_degenerate_and_isolated_vertices_in_the_lists():
    vert, tri = tc.messy()
    lists = tr.adjacency_literal(len(vert), tri)
    a = [int(r[0]) if r[0] == r[1] else int(r[1]) for r in tri if len(set(r.tolist())) == 2]
    assert len(a) == 1 and a[0] in lists[a[0]]                                  # (a, a, b) puts a into its own set
    iso = int(np.flatnonzero((vert == tc.MESSY_ISOLATED).all(1))[0])
    assert lists[iso] == [] and tr.incidence_literal(len(vert), tri)[iso] == []
    assert sum(len(x) for x in lists) < 2 * 3 * len(tri)                         # the duplicated triangle adds nothing


@pytest.mark.parametrize("name", sorted(tc.CASES))
@pytest.mark.parametrize("kind", (tr.SIMPLE, tr.LAPLACIAN, tr.TAUBIN))
def test_filters_literal_equals_vectorised(name, kind):
    """every case but the million-vertex grid; the hubs of the long fans are the long sequential sums, where np.add.at has to add
    in order"""
    vert, tri = tc.CASES[name]()
    nrm, col = tc.attributes(len(vert), 7)
    n = 1 if len(vert) >= BIG else 2
    a = tr.smooth(kind, vert, tri, n, normals=nrm, colors=col, literal=True)
    b = tr.smooth(kind, vert, tri, n, normals=nrm, colors=col)
    for x, y in zip(a, b):
        assert _same(x, y)
    assert not np.array_equal(b[0], vert)


@pytest.mark.parametrize("name", sorted(tc.CASES))
def test_vertex_normals_literal_equals_vectorised_and_the_package_helper(r3d, name):
    vert, tri = tc.CASES[name]()
    for raw in (False, True):
        assert _same(tr.vertex_normals(vert, tri, raw), tr.vertex_normals_literal(vert, tri, raw))
    assert _same(tr.vertex_normals(vert, tri), r3d.TriangleMesh(vert, tri).compute_vertex_normals().vertex_normals)


def test_scopes_and_copies():
    vert, tri = tc.noisy_sphere()
    nrm, col = tc.attributes(len(vert), 8)
    full = tr.smooth(tr.LAPLACIAN, vert, tri, 2, normals=nrm, colors=col)
    for scope, changed in ((tr.VERTEX, (True, False, False)), (tr.NORMAL, (False, True, False)), (tr.COLOR, (False, False, True))):
        got = tr.smooth(tr.LAPLACIAN, vert, tri, 2, scope=scope, normals=nrm, colors=col)
        for g, src, f, ch in zip(got, (vert, nrm, col), full, changed):
            assert not np.array_equal(g, src) if ch else _same(g, np.asarray(src))
        # colours and normals filtered alone use the weights of the unmoved positions: only the first step equals the full filter's
        one = tr.smooth(tr.LAPLACIAN, vert, tri, 1, scope=scope, normals=nrm, colors=col)
        first = tr.smooth(tr.LAPLACIAN, vert, tri, 1, normals=nrm, colors=col)
        assert all(_same(o, f1) for o, f1, ch in zip(one, first, changed) if ch)
    zero = tr.smooth(tr.TAUBIN, vert, tri, 0, normals=nrm, colors=col)
    assert _same(zero[0], np.asarray(vert)) and _same(zero[1], nrm) and _same(zero[2], col)
    with pytest.raises(ValueError):
        tr.smooth(tr.SIMPLE, vert, tri, -1)
    assert full[0].shape == vert.shape


def test_laplacian_shrinks_and_taubin_shrinks_less():
    vert, tri = tc.noisy_sphere()
    v0 = tr.enclosed_volume(vert, tri)
    lap = tr.enclosed_volume(tr.smooth(tr.LAPLACIAN, vert, tri, 5)[0], tri)
    tau = tr.enclosed_volume(tr.smooth(tr.TAUBIN, vert, tri, 5)[0], tri)
    print(f"enclosed volume {v0:.4f} -> Laplacian x5 {lap:.4f}, Taubin x5 {tau:.4f}")
    assert lap < v0 and abs(tau - v0) < abs(lap - v0)


def test_isolated_vertex_is_kept():
    vert, tri = tc.messy()
    iso = int(np.flatnonzero((vert == tc.MESSY_ISOLATED).all(1))[0])
    for kind in (tr.SIMPLE, tr.LAPLACIAN, tr.TAUBIN):
        for literal in (False, True):
            out = tr.smooth(kind, vert, tri, 3, literal=literal)[0]
            assert np.array_equal(out[iso], tc.MESSY_ISOLATED) and np.isfinite(out).all()


@pytest.mark.parametrize("kind", (tr.SIMPLE, tr.LAPLACIAN))
def test_nan_ring_grows_by_one_per_step(kind):
    vert, tri = tc.grid(70, 70)
    vert = vert.copy()
    seed = int(np.flatnonzero((np.abs(vert[:, 0] - 35) < 0.5) & (np.abs(vert[:, 1] - 35) < 0.5))[0])
    vert[seed, 1] = np.nan
    off, nbs = tr.adjacency(len(vert), tri)
    ring = np.zeros(len(vert), bool)
    ring[seed] = True
    for n in range(1, 4):
        grown = ring.copy()
        for v in np.flatnonzero(ring):
            grown[nbs[off[v]:off[v + 1]]] = True
        ring = grown
        out = tr.smooth(kind, vert, tri, n)[0]
        assert np.array_equal(np.isnan(out).any(1), ring), n
    assert 1 < ring.sum() < len(vert)


def test_compaction_rules():
    vert, tri = tc.messy()
    nv = len(vert)
    nrm, col = tc.attributes(nv, 9)
    v, t, n, c = tr.compact(vert, tri, tr.DROP_DEGENERATE, normals=nrm, colors=col)
    assert len(v) == nv and len(t) == len(tri) - 1 and _same(n, nrm) and _same(c, col)
    v, t, _, c = tr.compact(vert, tri, tr.DROP_UNREFERENCED, colors=col)
    assert len(v) == nv - 1 and len(t) == len(tri)                              # the degenerate triangle still references its vertices
    v, t, _, _ = tr.compact(vert, tri, tr.DROP_DEGENERATE | tr.DROP_UNREFERENCED)
    assert len(v) == nv - 2 and len(t) == len(tri) - 1
    assert np.array_equal(v[t], np.asarray(vert)[np.asarray(tri)[[len(set(r.tolist())) == 3 for r in tri]]])   # same corners, same order
    bad = np.asarray(vert).copy()
    bad[int(tri[0, 0]), 2] = np.inf
    v, t, _, _ = tr.compact(bad, tri, tr.DROP_NON_FINITE)
    assert len(v) == nv - 1 and np.isfinite(v).all() and len(t) == len(tri) - int((tri == tri[0, 0]).any(1).sum())
    v, t, _, _ = tr.compact(vert, tri, vertex_keep=np.zeros(nv, bool))
    assert v.shape == (0, 3) and t.shape == (0, 3)
    v, t, _, _ = tr.compact(vert, tri, vertex_keep=np.ones(nv, bool))
    assert _same(v, np.asarray(vert)) and np.array_equal(t, tri)
