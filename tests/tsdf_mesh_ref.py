"""numpy restatement of the triangle-mesh contract of the TSDF volume ("Triangle mesh"): Open3D's
ScalableTSDFVolume::ExtractTriangleMesh as recalled from 0.18, over the arrays ScalableTSDFVolume.debug_units() returns.  Two
forms, held equal bit for bit by tests/test_tsdf_mesh_ref.py: `mesh` works on all voxels at once, `mesh_literal` walks the cubes
one by one and keeps the vertices in a dict keyed by (lower voxel, axis), as Open3D keeps them in its unordered_map, and then
puts them into the package's order.  The triangle table is an argument: the tests pass the one the library was built with
(r3d_debug_mc_table), which tests/test_tsdf_mesh_ref.py checks by itself on all 256 rows.

Order.  Vertices: by owning voxel (units in ascending (X, Y, Z), voxels by flat index x*256 + y*16 + z), then axis x, y, z.
Triangles: by base voxel in the same order, then in the table's order."""
import numpy as np

R = 16
_LIMIT = 1 << 20
CORNERS = ((0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1))     # tests/tsdf_ref.py's _CORNERS
EDGE_CORNERS = ((0, 1), (1, 2), (3, 2), (0, 3), (4, 5), (5, 6), (7, 6), (4, 7), (0, 4), (1, 5), (2, 6), (3, 7))
EDGE_SHIFT = ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 0), (0, 0, 1), (1, 0, 1), (0, 1, 1), (0, 0, 1), (0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0))
EDGE_AXIS = (0, 1, 0, 1, 0, 1, 0, 1, 2, 2, 2, 2)


def _pack(U):
    U = np.asarray(U, dtype=np.int64)
    return ((U[..., 0] + _LIMIT) << 42) | ((U[..., 1] + _LIMIT) << 21) | (U[..., 2] + _LIMIT)


def _sorted_state(idx, tsdf, weight, colour):
    idx = np.asarray(idx, dtype=np.int64).reshape(-1, 3)
    n = len(idx)
    order = np.argsort(_pack(idx), kind="stable") if n else np.zeros(0, np.int64)
    T = np.asarray(tsdf, dtype=np.float32).reshape(n, R, R, R)[order]
    W = np.asarray(weight, dtype=np.float32).reshape(n, R, R, R)[order]
    C = None if colour is None else np.asarray(colour, dtype=np.float64).reshape(n, 3, R, R, R)[order]
    return idx[order], T, W, C


def _empty(colour):
    return np.zeros((0, 3)), (None if colour is None else np.zeros((0, 3))), np.zeros((0, 3), np.int32)


# ---- all voxels at once ------------------------------------------------------------------------------------------------------------
def mesh(idx, tsdf, weight, colour, vl, table):
    """-> vertices float64 [nv,3], colours float64 [nv,3] (None without colour), triangles int32 [nt,3]"""
    U, T, W, C = _sorted_state(idx, tsdf, weight, colour)
    n = len(U)
    if n == 0:
        return _empty(colour)
    table = np.asarray(table, dtype=np.int64).reshape(256, 16)
    count = (table >= 0).sum(1) // 3
    packed = _pack(U)

    def lookup(V):
        inr = ((V >= -_LIMIT) & (V < _LIMIT)).all(-1)
        key = _pack(V)
        pos = np.minimum(np.searchsorted(packed, key), n - 1)
        return np.where(inr & (packed[pos] == key), pos, -1)

    nbr = np.empty((n, 3, 3, 3), np.int64)      # the unit at U + d, d in {-1, 0, 1}^3, or -1
    for d in np.ndindex(3, 3, 3):
        nbr[(slice(None),) + d] = lookup(U + (np.array(d) - 1))
    ar = np.arange(R)

    def shifted(A, d, fill):
        """A [n,16,16,16] read at voxel + d for every voxel, `fill` where that voxel's unit is absent"""
        g = [ar + d[k] for k in range(3)]
        w = [gk // R + 1 for gk in g]
        m = [gk % R for gk in g]
        u = nbr[:, w[0][:, None, None], w[1][None, :, None], w[2][None, None, :]]
        val = A[np.maximum(u, 0), m[0][:, None, None], m[1][None, :, None], m[2][None, None, :]]
        return np.where(u >= 0, val, fill)

    present = np.ones((n, R, R, R), bool)
    active = np.ones((n, R, R, R), bool)
    index = np.zeros((n, R, R, R), np.int64)
    for i, off in enumerate(CORNERS):
        active &= shifted(present, off, False) & (shifted(W, off, np.float32(0)) != 0)
        index |= (shifted(T, off, np.float32(0)) < np.float32(0)).astype(np.int64) << i
    cube = np.where(active, index, 0)              # index 0 gives nothing, so an inactive cube may carry it

    exists = np.zeros((n, R, R, R, 3), bool)
    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3
        for q in range(4):
            d = [0, 0, 0]
            d[b], d[c] = q & 1, q >> 1
            B = shifted(cube, [-d[0], -d[1], -d[2]], 0)          # the cube this voxel is corner d of
            lo = CORNERS.index(tuple(d))
            d[a] = 1
            hi = CORNERS.index(tuple(d))
            exists[..., a] |= (((B >> lo) ^ (B >> hi)) & 1) != 0
    vid = np.where(exists, np.cumsum(exists.reshape(-1)).reshape(exists.shape) - 1, -1)
    ui, x, y, z, a = np.nonzero(exists)           # row-major: units, flat voxel index, axis
    nv = len(ui)
    h = U[ui] * R + np.stack([x, y, z], 1)
    eye = np.eye(3, dtype=np.int64)
    t_hi = np.empty(nv, np.float32)
    c_hi = None if C is None else np.empty((nv, 3))
    for k in range(3):
        sel = a == k
        t_hi[sel] = shifted(T, eye[k], np.float32(0))[ui[sel], x[sel], y[sel], z[sel]]
        if C is not None:
            for ch in range(3):
                c_hi[sel, ch] = shifted(C[:, ch], eye[k], 0.0)[ui[sel], x[sel], y[sel], z[sel]]
    f0, f1 = np.abs(T[ui, x, y, z].astype(np.float64)), np.abs(t_hi.astype(np.float64))
    p = 0.5 * vl + vl * h.astype(np.float64)
    rows = np.arange(nv)
    p[rows, a] = p[rows, a] + (f0 * vl) / (f0 + f1)
    colours = None
    if C is not None:
        c_lo = C[ui, :, x, y, z]
        colours = ((f1[:, None] * c_lo + f0[:, None] * c_hi) / (f0 + f1)[:, None]) / 255.0

    E = np.stack([shifted(vid[..., EDGE_AXIS[e]], EDGE_SHIFT[e], -1) for e in range(12)])       # [12, n,16,16,16]
    cu, cx, cy, cz = np.nonzero((cube != 0) & (cube != 255))
    cb = cube[cu, cx, cy, cz]
    Ec = E[:, cu, cx, cy, cz]                      # [12, cubes]
    parts, keys = [], []
    for k in range(5):
        sel = np.nonzero(count[cb] > k)[0]
        t = table[cb[sel]]
        parts.append(np.stack([Ec[t[:, 3 * k], sel], Ec[t[:, 3 * k + 2], sel], Ec[t[:, 3 * k + 1], sel]], 1))
        keys.append(sel * 5 + k)
    tri = np.concatenate(parts)[np.argsort(np.concatenate(keys), kind="stable")]
    return p, colours, tri.astype(np.int32).reshape(-1, 3)


# ---- cube by cube ------------------------------------------------------------------------------------------------------------------
def mesh_literal(idx, tsdf, weight, colour, vl, table):
    """The same, one cube at a time.  Only cubes whose eight tsdf signs are not all equal are visited (the others have index 0 or
    255 and give nothing, active or not): a 2x2x2 minimum / maximum over each unit and its neighbours finds them."""
    U, T, W, C = _sorted_state(idx, tsdf, weight, colour)
    if len(U) == 0:
        return _empty(colour)
    table = [[int(v) for v in row] for row in np.asarray(table).reshape(256, 16)]
    units = {tuple(int(v) for v in U[i]): i for i in range(len(U))}

    def unit_of(key):
        if any(k < -_LIMIT or k >= _LIMIT for k in key):
            return None
        return units.get(key)

    def voxel(g):
        """(unit number, x, y, z) of the global voxel g, None when its unit is absent"""
        i = unit_of(tuple(gk // R for gk in g))
        return None if i is None else (i, g[0] % R, g[1] % R, g[2] % R)

    vertex_of, vertices, colours, owners, triangles = {}, [], [], [], []
    for key in sorted(units):
        i = units[key]
        neg = np.zeros((R + 1, R + 1, R + 1), bool)           # signs of the corners 0..16, absent: positive
        for d in np.ndindex(2, 2, 2):
            j = unit_of((key[0] + d[0], key[1] + d[1], key[2] + d[2]))
            if j is not None:
                sl = tuple(slice(R, R + 1) if dk else slice(0, R) for dk in d)
                src = tuple(slice(0, 1) if dk else slice(0, R) for dk in d)
                neg[sl] = T[j][src] < 0
        s = np.zeros((R, R, R), np.int64)
        for off in CORNERS:
            s += neg[off[0]:off[0] + R, off[1]:off[1] + R, off[2]:off[2] + R]
        for x, y, z in np.argwhere((s > 0) & (s < 8)):
            g0 = (key[0] * R + int(x), key[1] * R + int(y), key[2] * R + int(z))
            index, active = 0, True
            for c, off in enumerate(CORNERS):
                at = voxel((g0[0] + off[0], g0[1] + off[1], g0[2] + off[2]))
                if at is None or W[at] == 0:
                    active = False
                    break
                if T[at] < np.float32(0):
                    index |= 1 << c
            if not active or index in (0, 255):
                continue
            row = table[index]
            for k in range(0, 15, 3):
                if row[k] < 0:
                    break
                ids = []
                for e in (row[k], row[k + 2], row[k + 1]):
                    lower = tuple(g0[m] + EDGE_SHIFT[e][m] for m in range(3))
                    axis = EDGE_AXIS[e]
                    if (lower, axis) not in vertex_of:
                        upper = tuple(lower[m] + (m == axis) for m in range(3))
                        lo, hi = voxel(lower), voxel(upper)
                        f0, f1 = abs(float(T[lo])), abs(float(T[hi]))
                        p = [0.5 * vl + vl * float(lower[m]) for m in range(3)]
                        p[axis] += (f0 * vl) / (f0 + f1)
                        vertex_of[(lower, axis)] = len(vertices)
                        vertices.append(p)
                        owners.append((tuple(lk // R for lk in lower), (lower[0] % R) * R * R + (lower[1] % R) * R + lower[2] % R, axis))
                        if C is not None:
                            colours.append([((f1 * float(C[lo[0], ch, lo[1], lo[2], lo[3]]) + f0 * float(C[hi[0], ch, hi[1], hi[2], hi[3]])) / (f0 + f1)) / 255.0
                                            for ch in range(3)])
                    ids.append(vertex_of[(lower, axis)])
                triangles.append(ids)
    # from the order of first use (Open3D's) to the package's
    order = sorted(range(len(vertices)), key=lambda v: owners[v])
    new_id = np.empty(len(vertices), np.int64)
    new_id[order] = np.arange(len(vertices))
    vert = np.array(vertices, dtype=np.float64).reshape(-1, 3)[order]
    col = None if C is None else np.array(colours, dtype=np.float64).reshape(-1, 3)[order]
    tri = new_id[np.array(triangles, dtype=np.int64).reshape(-1, 3)].astype(np.int32)
    return vert, col, tri


# ---- properties of a mesh ----------------------------------------------------------------------------------------------------------
def directed_edges(tri):
    """-> every directed edge of every triangle as a + b * 2^32, int64 [3 nt]"""
    t = np.asarray(tri, dtype=np.int64).reshape(-1, 3)
    return np.concatenate([t[:, 0] + (t[:, 1] << 32), t[:, 1] + (t[:, 2] << 32), t[:, 2] + (t[:, 0] << 32)])


def edge_census(tri):
    """-> (directed edges that occur more than once, directed edges whose reverse is absent, undirected edges)"""
    d = directed_edges(tri)
    uniq, cnt = np.unique(d, return_counts=True)
    rev = (uniq >> 32) + ((uniq & 0xFFFFFFFF) << 32)
    boundary = int((~np.isin(rev, uniq)).sum())
    undirected = len(np.unique(np.where((d >> 32) > (d & 0xFFFFFFFF), d, (d >> 32) + ((d & 0xFFFFFFFF) << 32))))
    return int((cnt > 1).sum()), boundary, undirected


def signed_volume(vert, tri):
    v0, v1, v2 = (vert[tri[:, k]] for k in range(3))
    return float((v0 * np.cross(v1, v2)).sum() / 6.0)
