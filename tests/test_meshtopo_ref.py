"""CPU tests of the mesh-topology contract's restatement (tests/meshtopo_ref.py): its literal and its vectorised form agree bit for bit,
facts that can be derived by hand hold, and the host-side helpers (component_mask, TriangleMesh's +=) do what they say (DESIGN.md
section 4, "Mesh topology")."""
import math

import numpy as np
import pytest

from tests import meshtopo_cases as mc
from tests import meshtopo_ref as mr
from tests import trimesh_cases as tc


def _same(a, b, what=""):
    assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), what


@pytest.mark.parametrize("name", sorted(mc.CASES))
def test_edges_and_components_literal_equals_vectorised(name):
    vert, tri = mc.CASES[name]()
    for got, want, what in zip(mr.edges(len(vert), tri), mr.edges_literal(len(vert), tri), ("edges", "counts", "stats")):
        _same(got, want, what)
    for got, want, what in zip(mr.components(vert, tri), mr.components_literal(vert, tri), ("labels", "counts", "areas")):
        _same(got, want, what)


# name: clusters, edges, boundary, non-manifold, characteristic (None: not derived)
FACTS = {
    "messy": (2, 11, 6, 2, 3),
    "tetrahedron": (1, 6, 0, 0, 2),
    "noisy_sphere": (1, 1080, None, None, 2),
    "grid70x70": (1, 14421, 276, None, 1),
    "fan5000": (1, 10000, None, None, 1),
}


@pytest.mark.parametrize("name", sorted(FACTS))
def test_facts_derivable_by_hand(name):
    vert, tri = mc.CASES[name]()
    clusters, n_edges, boundary, non_manifold, chi = FACTS[name]
    _, _, stats = mr.edges(len(vert), tri)
    labels, count, _ = mr.components(vert, tri)
    assert len(count) == clusters and labels.max() == clusters - 1 and count.sum() == len(tri)
    assert stats[0] == n_edges
    if boundary is not None:
        assert stats[1] == boundary
    if non_manifold is not None:
        assert stats[2] == non_manifold
    assert mr.euler_poincare_characteristic(len(vert), tri) == chi


def test_facts_of_the_new_cases():
    for p in mc.BOOKS:
        vert, tri = mc.book(p)
        edg, cnt, stats = mr.edges(len(vert), tri)
        assert stats.tolist() == [2 * p + 1, 2 * p, 1 if p > 2 else 0, 0] and cnt.max() == p
        assert len(mr.components(vert, tri)[1]) == 1
    assert len(mr.components(*mc.bowtie())[1]) == 2
    labels, count, _ = mr.components(*mc.soup(20_000))
    assert np.array_equal(labels, np.arange(20_000)) and (count == 1).all()
    for shuffled in (False, True):
        labels, count, _ = mr.components(*mc.strip(100_000, shuffled))
        assert count.tolist() == [100_000] and not labels.any()
    labels, count, area = mr.components(*mc.islands())
    assert len(count) == 54 and sorted(count.tolist())[-4:] == [720, 720, 4554, 4692] and (np.sort(count)[:50] == 1).all()
    assert area.max() / area.min() > 1e6


def test_the_two_million_vertex_grids():
    vert, tri = tc.big_grid()
    _, cnt, stats = mr.edges(len(vert), tri)
    assert stats.tolist() == [3_147_776, 4096, 0, 0]
    rounds = []
    labels, count, area = mr.components(vert, tri, rounds)
    assert count.tolist() == [len(tri)] and rounds[0] < 40
    terms = mr.area_terms(vert, tri)
    assert abs(area[0] - math.fsum(terms)) <= len(tri) * 2.0 ** -52 * math.fsum(terms)
    vert, tri = mc.cut_big_grid()
    labels, count, area = mr.components(vert, tri)
    assert len(count) == 2 and count.sum() == len(tri) and count.min() > 1_000_000
    assert labels[0] == 0 and set(np.unique(labels)) == {0, 1}


@pytest.mark.parametrize("name", sorted(mc.CASES))
def test_partition_equals_scipy(name):
    sp = pytest.importorskip("scipy.sparse")
    from scipy.sparse.csgraph import connected_components
    vert, tri = mc.CASES[name]()
    a, b = mr.links(len(vert), tri)
    n, theirs = connected_components(sp.coo_matrix((np.ones(len(a)), (a, b)), shape=(len(tri), len(tri))), directed=False)
    labels, count, _ = mr.components(vert, tri)
    assert n == len(count)
    # the same partition: their label is a function of ours and the other way round
    pairs = np.unique(np.stack([labels, theirs], 1), axis=0)
    assert len(pairs) == n


@pytest.mark.parametrize("name", sorted(mc.CASES))
def test_cluster_area_against_fsum(name):
    """n * 2**-52 relative is the bound for any fixed order of n non-negative terms: derived, not measured"""
    vert, tri = mc.CASES[name]()
    labels, count, area = mr.components(vert, tri)
    terms = mr.area_terms(vert, tri)
    order = np.argsort(labels, kind="stable")
    start = np.concatenate([[0], np.cumsum(count)])
    for c in range(0, len(count), max(1, len(count) // 60)):
        exact = math.fsum(terms[order[start[c]:start[c + 1]]].tolist())
        assert abs(area[c] - exact) <= count[c] * 2.0 ** -52 * exact, (name, c)


@pytest.mark.parametrize("name", sorted(mc.WELD_CASES) + sorted(mc.TRIANGLE_CASES))
@pytest.mark.parametrize("flags", (1, 2, 3))
def test_dedup_literal_equals_vectorised(name, flags):
    vert, tri, nrm, col = {**mc.WELD_CASES, **mc.TRIANGLE_CASES}[name]()
    got = mr.dedup(vert, tri, flags, nrm, col)
    want = mr.dedup_literal(vert, tri, flags, nrm, col)
    for g, w, what in zip(got, want, ("vertices", "triangles", "normals", "colours", "vertex_map", "triangle_origin")):
        _same(g, w, what)


def test_dedup_facts():
    vert, tri, nrm, col = mc.weld_soup70()
    ov, ot, on, oc, vmap, origin = mr.dedup(vert, tri, 1, nrm, col)
    assert len(ov) == 4900 and len(ot) == len(tri) and np.array_equal(ov[vmap], vert)
    first = np.array([np.flatnonzero(vmap == k)[0] for k in range(0, 4900, 97)])
    assert np.array_equal(on[::97], nrm[first]) and np.array_equal(oc[::97], col[first])       # the first occurrence's attributes
    assert len(mr.dedup(*mc.weld_copies()[:2], 1)[0]) == 1
    assert len(mr.dedup(*mc.weld_zeros()[:2], 1)[0]) == 1 + 3
    assert len(mr.dedup(*mc.weld_nans()[:2], 1)[0]) == 12 + 2
    assert len(mr.dedup(*mc.weld_bytes()[:2], 1)[0]) == 1 + 24 + 3
    vert, tri = mc.weld_soup300()[:2]
    assert len(vert) > 256 * 1024 and len(mr.dedup(vert, tri, 1)[0]) == 90_000
    assert mr.dedup(*mc.rotations()[:2], 2)[5].tolist() == [0, 3, 5, 8]
    assert len(mr.dedup(*mc.messy()[:2], 2)[1]) == 5
    for name in ("twice_sphere", "twice_grid"):
        vert, tri = mc.TRIANGLE_CASES[name]()[:2]
        ov, ot = mr.dedup(vert, tri, 3)[:2]
        assert (len(ov), len(ot)) == (len(vert) // 2, len(tri) // 2)
    vert, tri = mc.doubled_big_grid()
    assert tri.max() > 65535
    origin = mr.dedup(vert, tri, 2)[5]
    assert np.array_equal(origin, np.arange(len(tri) // 2))


def test_component_mask(r3d):
    labels = np.array([0, 0, 1, 2, 2, 2, 3, 3, 3], np.int32)
    count, area = np.array([2, 1, 3, 3]), np.array([5.0, 0.1, 0.2, 9.0])
    mo = r3d.mesh_ops
    for kw in (dict(), dict(min_triangles=2), dict(min_triangles=3), dict(min_area=1.0), dict(keep_largest=True), dict(min_area=0.15, keep_largest=True),
               dict(min_triangles=4, keep_largest=True)):
        got = mo.component_mask(labels, count, area, **kw)
        assert got.dtype == bool and np.array_equal(got, mr.component_mask(labels, count, area, **kw)), kw
    assert mo.component_mask(labels, count, area, keep_largest=True).tolist() == [True] * 3 + [False] * 3 + [True] * 3      # ties: the lower label
    assert mo.component_mask(labels, count, area, min_triangles=2).tolist() == [False, False, True] + [False] * 6
    assert len(mo.component_mask(np.zeros(0, np.int32), np.zeros(0, np.int64), np.zeros(0))) == 0


def test_iadd_and_add(r3d):
    va, ta = tc.tetrahedron()
    vb, tb = tc.two_triangles()
    na, ca = tc.attributes(len(va), 1)
    nb, cb = tc.attributes(len(vb), 2)
    a = r3d.TriangleMesh(va, ta, ca, na)
    b = r3d.TriangleMesh(vb, tb, cb, nb)
    c = a + b
    assert c is not a and len(a.vertices) == 4                                   # + leaves its operands alone
    assert np.array_equal(c.vertices, np.concatenate([va, vb])) and np.array_equal(c.triangles, np.concatenate([ta, tb + 4]))
    assert c.triangles.dtype == np.int32 and c.triangles.flags["C_CONTIGUOUS"]
    assert np.array_equal(c.vertex_colors, np.concatenate([ca, cb])) and np.array_equal(c.vertex_normals, np.concatenate([na, nb]))
    d = r3d.TriangleMesh(va, ta, ca) + b                                         # normals only on one side: dropped
    assert d.vertex_normals is None and np.array_equal(d.vertex_colors, np.concatenate([ca, cb]))
    e = r3d.TriangleMesh(va, ta, None, na)
    e.adjacency_list = [None] * 4
    same = e
    e += b
    assert e is same and e.vertex_colors is None and e.adjacency_list is None and len(e.vertex_normals) == 8
    f = r3d.TriangleMesh()                                                       # an empty mesh takes everything the other has
    f += b
    assert np.array_equal(f.vertices, vb) and np.array_equal(f.triangles, tb) and np.array_equal(f.vertex_colors, cb)
    g = r3d.TriangleMesh(va, ta, ca, na)
    g += r3d.TriangleMesh()
    assert len(g.vertices) == 4 and g.vertex_colors is not None
