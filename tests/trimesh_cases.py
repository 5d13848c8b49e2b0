"""Small meshes for the triangle-mesh tests, shared by tests/test_trimesh_ref.py (CPU) and tests/test_trimesh_gpu.py.  Every case is
(vertices float64 [n,3], triangles int32 [m,3]), cached and read-only.  Vertex numbering, triangle order and the starting corner
of every triangle are shuffled with a fixed seed, so no list arrives sorted; the orientation of every triangle is kept.

Sizes are chosen around the paths of csrc/trimesh.hip: a vertex in more than 32 corners is sorted by a workgroup (fans of 32 and
33), in LDS up to 4096 entries (corner lists: fans of 4096 and 4097; neighbour candidates, two per corner: fans of 2048 and 2049)
and in place beyond; the scan works in tiles of 4096 elements over nv + 1 counts (grids of 4095, 4096 and 4097 vertices, 70 x 70)
and adds up to 256 tile sums per thread round (1025 x 1025: 257 tiles)."""
import functools

import numpy as np


def _shuffled(vertices, triangles, seed):
    rng = np.random.default_rng(seed)
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    t = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    perm = rng.permutation(len(v))              # new number of old vertex i is perm[i]
    out_v = np.empty_like(v)
    out_v[perm] = v
    t = perm[t] if len(t) else t
    t = t[rng.permutation(len(t))]
    rot = rng.integers(0, 3, len(t))
    t = np.stack([t[np.arange(len(t)), (rot + c) % 3] for c in range(3)], 1) if len(t) else t
    out_v.setflags(write=False)
    t = np.ascontiguousarray(t, dtype=np.int32).reshape(-1, 3)
    t.setflags(write=False)
    return out_v, t


@functools.lru_cache(maxsize=None)
def tetrahedron():
    return _shuffled([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], [[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], 1)


@functools.lru_cache(maxsize=None)
def two_triangles():
    return _shuffled([[0, 0, 0], [1, 0, 0.1], [0, 1, 0.2], [1, 1.5, -0.1]], [[0, 1, 2], [2, 1, 3]], 2)


@functools.lru_cache(maxsize=None)
def messy():
    """a strip of four triangles, a triangle that occurs twice, a degenerate (a, a, b) triangle, a vertex only the degenerate
    triangle uses and a vertex no triangle uses"""
    vert = [[0, 0, 0], [1, 0, 0.3], [2, 0, -0.2], [0, 1, 0.1], [1, 1, 0.4], [2, 1, 0], [3, 3, 3], [-2, -1, 5]]
    tri = [[0, 1, 3], [1, 4, 3], [1, 2, 4], [2, 5, 4], [1, 2, 4], [4, 4, 6]]
    return _shuffled(vert, tri, 3)


MESSY_ISOLATED = np.array([-2.0, -1.0, 5.0])     # the position of messy()'s vertex without a triangle


@functools.lru_cache(maxsize=None)
def fan(spokes):
    """a closed fan: a hub above a wavy rim of `spokes` vertices, triangle i = (hub, rim i, rim i + 1)"""
    a = 2 * np.pi * np.arange(spokes) / spokes
    rng = np.random.default_rng(spokes)
    rim = np.stack([np.cos(a), np.sin(a), 0.1 * np.sin(5 * a)], 1) * (1 + 0.05 * rng.standard_normal((spokes, 1)))
    vert = np.concatenate([[[0.01, -0.02, 0.5]], rim])
    i = np.arange(spokes)
    tri = np.stack([np.zeros(spokes, np.int64), 1 + i, 1 + (i + 1) % spokes], 1)
    return _shuffled(vert, tri, 100 + spokes)


FANS = (32, 33, 63, 64, 65, 300, 2048, 2049, 4096, 4097, 5000)


@functools.lru_cache(maxsize=None)
def grid(w, h):
    """w x h vertices on a bumpy sheet, two triangles per cell"""
    rng = np.random.default_rng(w * 10007 + h)
    y, x = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    z = 0.3 * np.sin(0.37 * x) * np.cos(0.23 * y) + 0.1 * rng.standard_normal((h, w))
    vert = np.stack([x, y, z], -1).reshape(-1, 3)
    i = (np.arange(h - 1)[:, None] * w + np.arange(w - 1)[None, :]).reshape(-1)
    tri = np.concatenate([np.stack([i, i + 1, i + w], 1), np.stack([i + 1, i + w + 1, i + w], 1)])
    return _shuffled(vert, tri, w * 31 + h)


GRIDS = ((65, 63), (64, 64), (241, 17), (70, 70))        # 4095, 4096, 4097 and 4900 vertices
BIG_GRID = (1025, 1025)                                  # 1 050 625 vertices, 2 097 152 triangles


@functools.lru_cache(maxsize=None)
def noisy_sphere():
    """a UV sphere of 2 + 18 x 20 = 362 vertices, outward triangles, radius 1 with 3 % noise"""
    rings, seg = 18, 20
    th = np.pi * (1 + np.arange(rings)) / (rings + 1)
    ph = 2 * np.pi * np.arange(seg) / seg
    body = np.stack([np.sin(th)[:, None] * np.cos(ph)[None], np.sin(th)[:, None] * np.sin(ph)[None], np.cos(th)[:, None] * np.ones(seg)[None]], -1)
    vert = np.concatenate([[[0, 0, 1.0]], body.reshape(-1, 3), [[0, 0, -1.0]]])
    vert = vert * (1 + 0.03 * np.random.default_rng(362).standard_normal((len(vert), 1)))
    idx = lambda r, s: 1 + r * seg + (s % seg)      # noqa: E731
    tri = []
    for s in range(seg):
        tri.append([0, idx(0, s), idx(0, s + 1)])
        tri.append([len(vert) - 1, idx(rings - 1, s + 1), idx(rings - 1, s)])
        for r in range(rings - 1):
            tri.append([idx(r, s), idx(r + 1, s), idx(r + 1, s + 1)])
            tri.append([idx(r, s), idx(r + 1, s + 1), idx(r, s + 1)])
    assert len(vert) == 362
    return _shuffled(vert, tri, 362)


@functools.lru_cache(maxsize=None)
def tsdf_sphere():
    """the radius-11 sphere of tests/tsdf_mesh_cases.py as the marching-cubes restatement extracts it (2284 vertices), in the
    extraction's own order; -> vertices, triangles.  tsdf_sphere_colours() has its colours."""
    from tests import tsdf_mesh_cases as mc
    vert, _, tri = mc.reference("sphere")
    return np.ascontiguousarray(vert), np.ascontiguousarray(tri, dtype=np.int32)


def tsdf_sphere_colours():
    from tests import tsdf_mesh_cases as mc
    return np.ascontiguousarray(mc.reference("sphere")[1])


SMALL = dict(tetrahedron=tetrahedron, two_triangles=two_triangles, messy=messy, noisy_sphere=noisy_sphere, tsdf_sphere=tsdf_sphere)
SMALL.update({f"fan{n}": functools.partial(fan, n) for n in FANS})
SMALL.update({f"grid{w}x{h}": functools.partial(grid, w, h) for w, h in GRIDS})
# every case but the million-vertex grid
CASES = dict(SMALL)


def big_grid():
    return grid(*BIG_GRID)


def attributes(n, seed):
    """-> normals (unit rows) and colours in [0, 1] for n vertices"""
    rng = np.random.default_rng(seed)
    nrm = rng.standard_normal((n, 3))
    nrm /= np.sqrt((nrm * nrm).sum(1))[:, None]
    return nrm, rng.uniform(0.0, 1.0, (n, 3))
