"""The contract of the triangle-mesh operations ("Triangle-mesh operations") restated in numpy, twice:

* a literal form, vertex by vertex with Python loops (`*_literal`), and
* a vectorised form that sorts entries by (vertex, neighbour) and adds with np.add.at, which is unbuffered and therefore adds
  sequentially in that order.

tests/test_trimesh_ref.py holds the two equal bit for bit on the CPU; tests/test_trimesh_gpu.py holds the device to the vectorised
form.  Every floating-point expression is written in the order the contract gives, with parentheses where the order matters."""
import numpy as np

SIMPLE, LAPLACIAN, TAUBIN = 0, 1, 2
ALL, COLOR, NORMAL, VERTEX = 0, 1, 2, 3
DROP_DEGENERATE, DROP_UNREFERENCED, DROP_NON_FINITE = 1, 2, 4
KEEP_ISOLATED = True        # the one deviation from Open3D (which divides 0 / 0): a vertex with an empty adjacency set keeps its values


def _tri(triangles):
    return np.asarray(triangles, dtype=np.int64).reshape(-1, 3)


# ---- incidence and adjacency ---------------------------------------------------------------------------------------------------------
def incidence_literal(nv, triangles):
    """-> per vertex the list of corners 3 t + c with triangles[t][c] == v, ascending"""
    out = [[] for _ in range(nv)]
    for t, row in enumerate(_tri(triangles)):
        for c in range(3):
            out[int(row[c])].append(3 * t + c)
    return out


def incidence(nv, triangles):
    """-> offsets int32 [nv + 1], corners int32 (CSR)"""
    flat = _tri(triangles).reshape(-1)
    corners = np.argsort(flat, kind="stable").astype(np.int32)
    off = np.zeros(nv + 1, np.int64)
    np.cumsum(np.bincount(flat, minlength=nv), out=off[1:])
    return off.astype(np.int32), corners


def adjacency_literal(nv, triangles):
    """ComputeAdjacencyList with ordered sets: every triangle inserts each of its vertices into the sets of the other two (so a
    degenerate (a, a, b) puts a into its own set) -> per vertex the ascending list"""
    sets = [set() for _ in range(nv)]
    for a, b, c in _tri(triangles):
        a, b, c = int(a), int(b), int(c)
        sets[a].add(b)
        sets[a].add(c)
        sets[b].add(a)
        sets[b].add(c)
        sets[c].add(a)
        sets[c].add(b)
    return [sorted(s) for s in sets]


def adjacency(nv, triangles):
    """-> offsets int32 [nv + 1], neighbours int32 (CSR), entries sorted by (vertex, neighbour) without repeats"""
    t = _tri(triangles)
    v = np.concatenate([t[:, 0], t[:, 0], t[:, 1], t[:, 1], t[:, 2], t[:, 2]])
    nb = np.concatenate([t[:, 1], t[:, 2], t[:, 0], t[:, 2], t[:, 0], t[:, 1]])
    keys = np.unique(v * max(nv, 1) + nb)
    off = np.zeros(nv + 1, np.int64)
    np.cumsum(np.bincount(keys // max(nv, 1), minlength=nv), out=off[1:])
    return off.astype(np.int32), (keys % max(nv, 1)).astype(np.int32)


def csr_to_lists(off, entries):
    return [[int(x) for x in entries[off[v]:off[v + 1]]] for v in range(len(off) - 1)]


# ---- one smoothing step --------------------------------------------------------------------------------------------------------------
def step_literal(kind, pos, attrs, adj_lists, lam):
    """one step (kind SIMPLE or LAPLACIAN) of every array in attrs, weights from pos -> list of new arrays"""
    outs = [a.copy() for a in attrs]
    for v, nbs in enumerate(adj_lists):
        if not nbs and KEEP_ISOLATED:
            continue
        if kind == SIMPLE:
            for a, o in zip(attrs, outs):
                s = a[v].copy()
                for nb in nbs:
                    s = s + a[nb]
                o[v] = s / float(len(nbs) + 1)
            continue
        tw = 0.0
        sums = [np.zeros(3) for _ in attrs]
        with np.errstate(all="ignore"):
            for nb in nbs:
                d = pos[v] - pos[nb]
                dist = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
                w = 1.0 / (dist + 1e-12)
                tw = tw + w
                for a, s in zip(attrs, sums):
                    s += w * a[nb]
            for a, s, o in zip(attrs, sums, outs):
                o[v] = a[v] + lam * (s / tw - a[v])
    return outs


def step(kind, pos, attrs, off, nbs, lam):
    """the same, vectorised over the CSR adjacency"""
    nv = len(pos)
    deg = np.diff(off.astype(np.int64))
    rows = np.repeat(np.arange(nv), deg)
    nb = nbs.astype(np.int64)
    has = (deg > 0) if KEEP_ISOLATED else np.ones(nv, bool)
    outs = []
    with np.errstate(all="ignore"):
        if kind == LAPLACIAN:
            d = pos[rows] - pos[nb]
            dist = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
            w = 1.0 / (dist + 1e-12)
            tw = np.zeros(nv)
            np.add.at(tw, rows, w)
        for a in attrs:
            if kind == SIMPLE:
                acc = a.copy()
                np.add.at(acc, rows, a[nb])
                new = acc / (deg + 1).astype(np.float64)[:, None]
            else:
                s = np.zeros((nv, 3))
                np.add.at(s, rows, w[:, None] * a[nb])
                new = a + lam * (s / tw[:, None] - a)
            outs.append(np.where(has[:, None], new, a))
    return outs


def smooth(kind, vertices, triangles, iterations, lam=0.5, mu=-0.53, scope=ALL, normals=None, colors=None, literal=False):
    """filter_smooth_simple / _laplacian / _taubin -> (vertices, normals or None, colours or None), new arrays"""
    if iterations < 0:
        raise ValueError("negative iterations")
    pos = np.array(vertices, dtype=np.float64).reshape(-1, 3)
    nrm = None if normals is None else np.array(normals, dtype=np.float64).reshape(-1, 3)
    col = None if colors is None else np.array(colors, dtype=np.float64).reshape(-1, 3)
    nv = len(pos)
    if literal:
        lists = adjacency_literal(nv, triangles)
    else:
        off, nbs = adjacency(nv, triangles)
    f_pos = scope in (ALL, VERTEX)
    f_nrm = nrm is not None and scope in (ALL, NORMAL)
    f_col = col is not None and scope in (ALL, COLOR)
    lams = [lam, mu] if kind == TAUBIN else [lam]
    base = SIMPLE if kind == SIMPLE else LAPLACIAN
    for _ in range(iterations):
        for l in lams:
            attrs = [a for a, f in ((pos, f_pos), (nrm, f_nrm), (col, f_col)) if f]
            if not attrs:
                continue
            new = step_literal(base, pos, attrs, lists, l) if literal else step(base, pos, attrs, off, nbs, l)
            new = iter(new)
            if f_pos:
                pos = next(new)
            if f_nrm:
                nrm = next(new)
            if f_col:
                col = next(new)
    return pos, nrm, col


# ---- normals -------------------------------------------------------------------------------------------------------------------------
def _faces(vertices, triangles):
    v, t = np.asarray(vertices, dtype=np.float64).reshape(-1, 3), _tri(triangles)
    if not len(t):
        return np.zeros((0, 3))
    return np.cross(v[t[:, 1]] - v[t[:, 0]], v[t[:, 2]] - v[t[:, 0]])


def _normalised(n):
    length = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
    with np.errstate(all="ignore"):
        return np.where(length[:, None] != 0, n / length[:, None], n)


def triangle_normals(vertices, triangles, raw=False):
    n = _faces(vertices, triangles)
    return n if raw else _normalised(n)


def vertex_normals(vertices, triangles, raw=False):
    """the cross products added in ascending corner order (np.add.at over the corners in order), then normalised"""
    t = _tri(triangles)
    n = np.zeros((len(np.asarray(vertices).reshape(-1, 3)), 3))
    if len(t):
        np.add.at(n, t.reshape(-1), np.repeat(_faces(vertices, triangles), 3, axis=0))
    return n if raw else _normalised(n)


def vertex_normals_literal(vertices, triangles, raw=False):
    v, t = np.asarray(vertices, dtype=np.float64).reshape(-1, 3), _tri(triangles)
    out = np.zeros((len(v), 3))
    for i, corners in enumerate(incidence_literal(len(v), t)):
        s = np.zeros(3)
        for c in corners:
            a, b, cc = t[c // 3]
            e1, e2 = v[b] - v[a], v[cc] - v[a]
            s = s + np.array([e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]])
        if not raw:
            length = np.sqrt((s[0] * s[0] + s[1] * s[1]) + s[2] * s[2])
            if length != 0:
                s = s / length
        out[i] = s
    return out


# ---- clean-ups -----------------------------------------------------------------------------------------------------------------------
def compact(vertices, triangles, flags=0, vertex_keep=None, triangle_keep=None, normals=None, colors=None):
    """index arithmetic: triangles are decided first (mask, degenerate rule, no corner at a vertex its mask or the non-finite rule
    removes); "referenced" means referenced by a surviving triangle; survivors keep their order
    -> (vertices, triangles int32, normals or None, colours or None)"""
    v, t = np.asarray(vertices, dtype=np.float64).reshape(-1, 3), _tri(triangles)
    nv = len(v)
    gone = np.zeros(nv, bool) if vertex_keep is None else ~(np.asarray(vertex_keep).reshape(-1) != 0)
    if flags & DROP_NON_FINITE:
        gone = gone | ~np.isfinite(v).all(1)
    tk = np.ones(len(t), bool) if triangle_keep is None else (np.asarray(triangle_keep).reshape(-1) != 0)
    if flags & DROP_DEGENERATE:
        tk = tk & ~((t[:, 0] == t[:, 1]) | (t[:, 1] == t[:, 2]) | (t[:, 0] == t[:, 2]))
    tk = tk & ~gone[t].any(1) if len(t) else tk
    vk = ~gone
    if flags & DROP_UNREFERENCED:
        ref = np.zeros(nv, bool)
        ref[t[tk].reshape(-1)] = True
        vk = vk & ref
    remap = np.cumsum(vk) - 1
    pick = lambda a: None if a is None else np.asarray(a, dtype=np.float64).reshape(-1, 3)[vk]    # noqa: E731
    return v[vk], remap[t[tk]].astype(np.int32).reshape(-1, 3), pick(normals), pick(colors)


def enclosed_volume(vertices, triangles):
    v, t = np.asarray(vertices, dtype=np.float64), _tri(triangles)
    return abs(float((v[t[:, 0]] * np.cross(v[t[:, 1]], v[t[:, 2]])).sum()) / 6.0)
