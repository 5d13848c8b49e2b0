"""CPU tests of what the triangle-mesh tests rest on: the marching-cubes table the library was built with (r3d_debug_mc_table),
checked by itself on all 256 rows, and the numpy restatement tests/tsdf_mesh_ref.py, whose two forms must agree bit for bit on
every case of tests/tsdf_mesh_cases.py and give the counts pinned there."""
import numpy as np
import pytest

from tests import tsdf_mesh_cases as mc
from tests import tsdf_mesh_ref as mr

FACES = [(axis, side) for axis in range(3) for side in (0, 1)]


@pytest.fixture(scope="module")
def table(r3d):
    t = r3d.tsdf.mc_table()
    assert t.shape == (256, 16) and t.dtype == np.int8
    return [[int(v) for v in row] for row in t]


def _triples(row):
    n = row.index(-1)
    assert n % 3 == 0 and all(v == -1 for v in row[n:]), "entries come in triples, -1 to the end"
    return [tuple(row[k:k + 3]) for k in range(0, n, 3)]


def _crossing(r):
    return {e for e, (a, b) in enumerate(mr.EDGE_CORNERS) if ((r >> a) ^ (r >> b)) & 1}


def _in_face(e, face):
    return all(mr.CORNERS[c][face[0]] == face[1] for c in mr.EDGE_CORNERS[e])


def _boundary(triples):
    """directed edges (pairs of cube edges) of the row's triangles whose reverse is absent"""
    directed = [(t[k], t[(k + 1) % 3]) for t in triples for k in range(3)]
    assert len(set(directed)) == len(directed), "a directed triangle edge occurs twice"
    return [d for d in directed if (d[1], d[0]) not in directed]


def test_table_is_the_classic_one(table):
    assert table[1][:4] == [0, 8, 3, -1] and table[3][:7] == [1, 8, 3, 9, 8, 1, -1]
    assert sum(len(_triples(row)) for row in table) == 820


def test_rows_use_exactly_the_crossing_edges(table):
    for r, row in enumerate(table):
        triples = _triples(row)
        assert len(triples) <= 5
        assert all(0 <= e < 12 for t in triples for e in t)
        assert {e for t in triples for e in t} == _crossing(r), f"row {r}"
    assert _triples(table[0]) == [] and _triples(table[255]) == []


def test_rows_close_up_inside_the_cube(table):
    """every directed edge once; an edge without its reverse lies in exactly one cube face, and on every face every crossing edge
    of the face ends exactly one such segment"""
    for r, row in enumerate(table):
        segments = _boundary(_triples(row))
        on_face = {face: [] for face in FACES}
        for a, b in segments:
            faces = [f for f in FACES if _in_face(a, f) and _in_face(b, f)]
            assert a != b and len(faces) == 1, f"row {r}: the segment {a}-{b} lies in {len(faces)} faces"
            on_face[faces[0]].append((a, b))
        for face in FACES:
            ends = [e for seg in on_face[face] for e in seg]
            assert sorted(ends) == sorted(e for e in _crossing(r) if _in_face(e, face)), f"row {r}, face {face}"


def test_neighbouring_cubes_meet_on_their_face(table):
    """per axis and per mixed sign pattern of a face's four corners: the same segments whichever row produces them, on the low
    face and on the high face (a cube's high face is its neighbour's low face), and run through in opposite directions there, so
    that the two cubes' triangles join with one orientation"""
    def project(e, axis):
        return frozenset(tuple(v for k, v in enumerate(mr.CORNERS[c]) if k != axis) for c in mr.EDGE_CORNERS[e])

    seen = {}
    for r, row in enumerate(table):
        segments = _boundary(_triples(row))
        for axis, side in FACES:
            corners = [c for c in range(8) if mr.CORNERS[c][axis] == side]
            pattern = tuple((r >> c) & 1 for c in sorted(corners, key=lambda c: tuple(v for k, v in enumerate(mr.CORNERS[c]) if k != axis)))
            if len(set(pattern)) == 1:
                continue
            on = [(project(a, axis), project(b, axis)) for a, b in segments if _in_face(a, (axis, side)) and _in_face(b, (axis, side))]
            undirected = frozenset(frozenset(s) for s in on)
            directed = frozenset(on if side == 0 else [(b, a) for a, b in on])
            assert seen.setdefault((axis, pattern), (undirected, directed)) == (undirected, directed), f"row {r}, axis {axis}, side {side}, pattern {pattern}"
    assert len(seen) == 3 * 14


def test_orientation_on_a_small_sphere(table):
    """a sphere of radius 4.2 voxels at (6.3, 6.6, 7.1) in a 14^3 lattice of weight 1 (voxel length 1, so positions are voxel
    index + 0.5): closed, Euler characteristic 2, faces outward; the surface is inscribed in the sphere, so its volume is below"""
    g = np.stack(np.meshgrid(np.arange(16), np.arange(16), np.arange(16), indexing="ij"), -1).astype(np.float64)
    centre, radius = np.array([6.3, 6.6, 7.1]), 4.2
    tsdf = (np.sqrt((((g + 0.5) - (centre + 0.5)) ** 2).sum(-1)) - radius).astype(np.float32)
    weight = np.zeros((16, 16, 16), np.float32)
    weight[:14, :14, :14] = 1
    vert, col, tri = mr.mesh_literal(np.zeros((1, 3), np.int32), tsdf.reshape(1, -1), weight.reshape(1, -1), None, 1.0, table)
    repeated, boundary, undirected = mr.edge_census(tri)
    ratio = mr.signed_volume(vert, tri) / (4.0 / 3.0 * np.pi * radius ** 3)
    print(f"{len(vert)} vertices, {len(tri)} triangles, volume ratio {ratio:.4f}")
    assert col is None and repeated == 0 and boundary == 0
    assert len(vert) - undirected + len(tri) == 2
    assert 0.9 < ratio < 1.0
    assert (len(vert), len(tri)) == (334, 664)
    assert np.abs(np.sqrt(((vert - (centre + 0.5)) ** 2).sum(1)) - radius).max() < 0.1       # linear interpolation of a distance field


@pytest.mark.parametrize("name", list(mc.CASES))
def test_forms_agree_and_counts_are_pinned(r3d, name):
    state = mc.CASES[name]()
    table = r3d.tsdf.mc_table()
    vert, col, tri = mc.reference(name)
    assert (len(vert), len(tri)) == mc.COUNTS[name] and len(tri) > 0
    lv, lc, lt = mr.mesh_literal(*state, mc.VL, table)
    assert vert.tobytes() == lv.tobytes() and col.tobytes() == lc.tobytes() and tri.tobytes() == lt.tobytes()
    assert tri.dtype == np.int32 and tri.min() >= 0 and tri.max() < len(vert) and len(np.unique(tri)) == len(vert)
    assert np.isfinite(vert).all() and np.isfinite(col).all() and col.min() >= 0.0 and col.max() <= 1.0
    if name in ("configurations", "plane"):       # the cases that also run without colour: the same mesh
        v2, c2, t2 = mc.reference(name, False)
        assert c2 is None and v2.tobytes() == vert.tobytes() and t2.tobytes() == tri.tobytes()


def test_configurations_have_the_tables_counts(r3d, table):
    """block k of the case is one active cube: its triangles are row k's"""
    vert, _, tri = mc.reference("configurations")
    base = np.floor(vert[tri[:, 0]] / mc.VL - 0.5 + 1e-9).astype(int)      # the lower voxel of the vertex's edge: inside the block
    block = (base[:, 0] + 16) // 3 + 8 * ((base[:, 1] + 16) // 3) + 64 * (base[:, 2] // 3)
    assert np.array_equal(np.bincount(block, minlength=256), [len(_triples(row)) for row in table])


def test_empty_state_gives_an_empty_mesh(table):
    for fn in (mr.mesh, mr.mesh_literal):
        vert, col, tri = fn(np.zeros((0, 3), np.int32), np.zeros((0, 4096), np.float32), np.zeros((0, 4096), np.float32), None, mc.VL, table)
        assert vert.shape == (0, 3) and tri.shape == (0, 3) and col is None
        zero = fn(np.zeros((1, 3), np.int32), np.ones((1, 4096), np.float32), np.zeros((1, 4096), np.float32), np.zeros((1, 3, 4096)), mc.VL, table)
        assert len(zero[0]) == 0 and len(zero[2]) == 0 and zero[1].shape == (0, 3)
