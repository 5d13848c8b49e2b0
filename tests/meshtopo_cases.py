"""Meshes for the mesh-topology tests, shared by tests/test_meshtopo_ref.py (CPU) and tests/test_meshtopo_gpu.py, next to those of
tests/trimesh_cases.py (imported, not edited).  Every case is cached and read-only, and shuffled with trimesh_cases._shuffled where
order should not help.

Sizes follow the paths of csrc/meshtopo.hip and the radix sort under it: runs of equal keys across lanes (64), waves and radix
tiles of 1024 items (books of 3 to 5000 triangles on one edge); long parent chains (a strip of 100 000 triangles, numbered along
the strip and shuffled); as many clusters as triangles past four 4096-element scan tiles (a soup of 20 000); components whose
areas differ by orders of magnitude (islands); lists of a million triangles for the upper level of the area sum (the cut grid);
more than 256 radix tiles of vertices (the soup of a 300 x 300 grid)."""
import functools

import numpy as np

from tests import trimesh_cases as tc

BOOKS = (3, 64, 65, 1025, 5000)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def book(p):
    """p triangles on the one edge (0, 1)"""
    a = 2 * np.pi * np.arange(p) / p
    vert = np.concatenate([[[0, 0, 0], [0, 0, 1.0]], np.stack([np.cos(a), np.sin(a), 0.5 + 0.1 * np.sin(3 * a)], 1)])
    tri = np.stack([np.zeros(p, np.int64), np.ones(p, np.int64), 2 + np.arange(p)], 1)
    return tc._shuffled(vert, tri, 7000 + p)


@functools.lru_cache(maxsize=None)
def bowtie():
    """two triangles that share one vertex: two clusters"""
    return tc._shuffled([[0, 0, 0], [1, 1, 0.1], [1, -1, 0.2], [-1, 1, 0.3], [-1, -1, -0.1]], [[0, 1, 2], [0, 3, 4]], 71)


def _strip(n):
    i = np.arange(n + 2, dtype=np.float64)
    vert = np.stack([0.5 * i, i % 2, 0.05 * np.sin(0.01 * i)], 1)
    k = np.arange(n)
    tri = np.where((k % 2 == 0)[:, None], np.stack([k, k + 1, k + 2], 1), np.stack([k + 1, k, k + 2], 1))
    return vert, tri


@functools.lru_cache(maxsize=None)
def strip(n, shuffled):
    """n triangles in a row, triangle k on vertices k, k + 1, k + 2: numbered along the strip, or shuffled"""
    vert, tri = _strip(n)
    if shuffled:
        return tc._shuffled(vert, tri, 7100 + n)
    return _frozen(np.ascontiguousarray(vert), np.ascontiguousarray(tri, dtype=np.int32))


@functools.lru_cache(maxsize=None)
def soup(n):
    """n isolated triangles"""
    rng = np.random.default_rng(7200 + n)
    centre = rng.uniform(-50, 50, (n, 1, 3))
    vert = (centre + rng.uniform(-0.5, 0.5, (n, 3, 3))).reshape(-1, 3)
    return tc._shuffled(vert, np.arange(3 * n).reshape(n, 3), 7300 + n)


def _join(parts, seed):
    verts, tris, off = [], [], 0
    for v, t in parts:
        verts.append(np.asarray(v, dtype=np.float64))
        tris.append(np.asarray(t, dtype=np.int64) + off)
        off += len(v)
    return tc._shuffled(np.concatenate(verts), np.concatenate(tris), seed)


def _without_vertices(vert, tri, gone):
    return vert, tri[~gone[tri].any(1)]


@functools.lru_cache(maxsize=None)
def islands():
    """grid(70, 70) without the triangles that touch column 35 (two half-grids), two noisy spheres at an offset and 50 lone triangles
    a hundredth of a cell wide: 54 clusters"""
    gv, gt = tc.grid(70, 70)
    sv, st = tc.noisy_sphere()
    rng = np.random.default_rng(7400)
    lone = (rng.uniform(0, 60, (50, 1, 3)) + [0, 0, 30] + rng.uniform(-0.01, 0.01, (50, 3, 3))).reshape(-1, 3)
    return _join([_without_vertices(gv, gt, gv[:, 0] == 35), (sv + [100, 0, 0], st), (3 * sv + [100, 10, 0], st), (lone, np.arange(150).reshape(50, 3))], 7401)


@functools.lru_cache(maxsize=None)
def cut_big_grid():
    """the 1025 x 1025 grid without the triangles that touch row 512: two clusters of about a million triangles"""
    v, t = tc.big_grid()
    t = np.ascontiguousarray(t[~(v[:, 1] == 512)[t].any(1)])
    t.setflags(write=False)
    return v, t


COMPONENT_CASES = {f"book{p}": functools.partial(book, p) for p in BOOKS}
COMPONENT_CASES.update(bowtie=bowtie, strip_natural=functools.partial(strip, 100_000, False), strip_shuffled=functools.partial(strip, 100_000, True),
                       soup20000=functools.partial(soup, 20_000), islands=islands)
# every mesh of trimesh_cases and every new one but the two of a million vertices
CASES = dict(tc.CASES)
CASES.update(COMPONENT_CASES)
BIG_CASES = dict(big_grid=tc.big_grid, cut_big_grid=cut_big_grid)
SLOW_LITERAL = ("strip_natural", "strip_shuffled")      # the literal forms still run on these; listed for the reader


# ---- welding cases: (vertices, triangles, normals, colours) ------------------------------------------------------------------------------
def soup_of(vert, tri, seed):
    """every triangle gets its own three vertices, then the numbering is shuffled"""
    t = np.asarray(tri, dtype=np.int64)
    return tc._shuffled(np.asarray(vert)[t.reshape(-1)], np.arange(3 * len(t)).reshape(-1, 3), seed)


def _with_attributes(vert, tri, seed):
    nrm, col = tc.attributes(len(vert), seed)
    return _frozen(np.ascontiguousarray(vert, dtype=np.float64), np.ascontiguousarray(tri, dtype=np.int32).reshape(-1, 3), nrm, col)


def _fan_over(n):
    """n - 2 triangles over n vertices, so that every case has triangles to renumber"""
    k = np.arange(max(n - 2, 0))
    return np.stack([np.zeros_like(k), k + 1, k + 2], 1)


@functools.lru_cache(maxsize=None)
def weld_soup70():
    return _with_attributes(*soup_of(*tc.grid(70, 70), 7500), 7501)


@functools.lru_cache(maxsize=None)
def weld_soup300():
    return _with_attributes(*soup_of(*tc.grid(300, 300), 7502), 7503)


@functools.lru_cache(maxsize=None)
def weld_copies():
    vert = np.tile([[0.25, -3.5, 1e-3]], (5000, 1))
    return _with_attributes(vert, _fan_over(5000), 7504)


@functools.lru_cache(maxsize=None)
def weld_zeros():
    """+0.0 against -0.0 in each coordinate: the eight sign patterns of (0, 0, 0) are one vertex, and so are the two of every row with
    one zero"""
    z = np.array([[sx * 0.0, sy * 0.0, sz * 0.0] for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)])
    one = np.array([[0.0, 1, 2], [-0.0, 1, 2], [1, 0.0, 2], [1, -0.0, 2], [1, 2, 0.0], [1, 2, -0.0]])
    vert = np.concatenate([z, one])
    return _with_attributes(vert, _fan_over(len(vert)), 7505)


@functools.lru_cache(maxsize=None)
def weld_nans():
    """rows with a NaN in each position, each three times, between rows that do weld"""
    rows = [[np.nan, 1, 2], [1, np.nan, 2], [1, 2, np.nan], [np.nan, np.nan, np.nan], [1, 2, 3], [4, 5, 6]]
    vert = np.array(rows * 3, dtype=np.float64)
    return _with_attributes(vert, _fan_over(len(vert)), 7506)


@functools.lru_cache(maxsize=None)
def weld_bytes():
    """a row twice, and for each of the 24 key bytes a row, twice, that differs from it in that byte alone (among them the lowest
    mantissa bit of z, the sign of x and the top exponent byte of y): every radix pass decides something"""
    base = np.array([1.2345678901234567, -2.3456789012345678, 3.4567890123456789])
    rows = [base, base]
    for byte in range(24):
        bits = base.view(np.uint64).copy()
        bits[byte // 8] ^= np.uint64(1 if byte % 8 != 7 else 0x80) << np.uint64(8 * (byte % 8))      # bit 0 of the byte; the sign in the top one
        rows += [bits.view(np.float64), bits.view(np.float64)]
    for axis in range(3):                                   # and bit 0 of the top exponent byte (bit 56), which the sign flip leaves alone
        bits = base.view(np.uint64).copy()
        bits[axis] ^= np.uint64(1) << np.uint64(56)
        rows += [bits.view(np.float64), bits.view(np.float64)]
    vert = np.array(rows)
    assert np.isfinite(vert).all()
    vert = vert[np.random.default_rng(7507).permutation(len(vert))]
    return _with_attributes(vert, _fan_over(len(vert)), 7508)


@functools.lru_cache(maxsize=None)
def weld_random(n):
    """n vertices drawn from n // 3 + 1 positions"""
    rng = np.random.default_rng(7600 + n)
    pool = rng.standard_normal((n // 3 + 1, 3))
    vert = pool[rng.integers(0, len(pool), n)]
    return _with_attributes(vert, _fan_over(n), 7700 + n)


WELD_CASES = dict(soup70=weld_soup70, copies=weld_copies, zeros=weld_zeros, nans=weld_nans, bytes=weld_bytes)
WELD_CASES.update({f"random{n}": functools.partial(weld_random, n) for n in (1023, 1024, 1025)})
WELD_BIG = dict(soup300=weld_soup300)


# ---- triangle duplicates ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def rotations():
    """a triangle, its two rotations, its flip and the flip's rotation, and a degenerate pair: (a,b,c), (b,c,a), (c,a,b) are one key,
    (a,c,b) and (c,b,a) another; (a,a,b) and (a,b,a) are rotations of one another"""
    vert = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1.0]])
    tri = [[0, 1, 2], [1, 2, 0], [2, 0, 1], [0, 2, 1], [2, 1, 0], [3, 3, 1], [3, 1, 3], [1, 3, 3], [3, 1, 1]]
    return _with_attributes(vert, tri, 7800)


@functools.lru_cache(maxsize=None)
def messy():
    return _with_attributes(*tc.messy(), 7801)


@functools.lru_cache(maxsize=None)
def doubled_big_grid():
    """the big grid followed by a rotated copy of itself: indices above 65 535, every second-half triangle a duplicate"""
    vert, tri = tc.big_grid()
    both = np.ascontiguousarray(np.concatenate([tri, tri[:, [1, 2, 0]]]))
    both.setflags(write=False)
    return vert, both


@functools.lru_cache(maxsize=None)
def twice(name):
    """mesh + mesh: welded with both flags it must return the original counts"""
    vert, tri = tc.CASES[name]()
    n = len(vert)
    return _with_attributes(np.concatenate([vert, vert]), np.concatenate([tri, tri[:, [2, 0, 1]] + n]), 7900)


TRIANGLE_CASES = dict(rotations=rotations, messy=messy, twice_sphere=functools.partial(twice, "noisy_sphere"), twice_grid=functools.partial(twice, "grid70x70"))
