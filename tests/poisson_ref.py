"""numpy restatement of the Poisson reconstruction contract ("Poisson reconstruction"), written from the
contract and not from the kernels.  Every stage exists twice and tests/test_poisson_ref.py holds the two forms equal bit for bit:
the `*_literal` functions walk nodes, points and cubes one by one in Python; the others work on whole arrays (np.add.at over
entries sorted by node, cell offset and point number applies them in order, so a node's sum runs in the contract's order).

Fields are float64 arrays of shape (G, G, G) indexed [k, j, i]: C order is the contract's linear index (k G + j) G + i.  Vector
fields carry the component first: (3, G, G, G)."""
import numpy as np

from tests.tsdf_mesh_ref import CORNERS, EDGE_AXIS, EDGE_SHIFT

DEFAULTS = dict(depth=8, cycles=10, pre=2, post=2, coarse_sweeps=40, scale=1.1, alpha=4.0, omega=0.8)


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


# ---- grid and cells -------------------------------------------------------------------------------------------------------------------
def grid(points, depth, scale):
    """-> org float64 [3], h, R, G"""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    lo, hi = p.min(0), p.max(0)
    c = (lo + hi) / 2.0
    s = scale * (hi - lo).max()
    R = 1 << depth
    return c - s / 2.0, s / R, R, R + 1


def cells(points, org, h, R):
    """-> cell int64 [n,3] (x, y, z), fractions float64 [n,3]"""
    g = (np.asarray(points, dtype=np.float64).reshape(-1, 3) - org) / h
    cell = np.clip(np.floor(g), 0, R - 1).astype(np.int64)
    return cell, g - cell


def _corner_weight(f, d):
    """((wx wy) wz) for corner d = (dx, dy, dz) of a cell, f [..., 3]"""
    w = [f[..., a] if d[a] else 1.0 - f[..., a] for a in range(3)]
    return (w[0] * w[1]) * w[2]


# ---- splats ---------------------------------------------------------------------------------------------------------------------------
def _gather(cell, f, wt, attr, G):
    """sum over the entries (point, corner) sorted by (node, rank of the cell offset, point) -> s0 (G,G,G), s3 (3,G,G,G) or None"""
    n = len(cell)
    node, rank, point, w = [], [], [], []
    for dz in range(2):
        for dy in range(2):
            for dx in range(2):
                node.append(((cell[:, 2] + dz) * G + cell[:, 1] + dy) * G + cell[:, 0] + dx)
                rank.append(np.full(n, (1 - dz) * 4 + (1 - dy) * 2 + (1 - dx)))      # the cell's offset from the node is -d
                point.append(np.arange(n))
                w.append(_corner_weight(f, (dx, dy, dz)) * wt)
    node, rank, point, w = (np.concatenate(a) for a in (node, rank, point, w))
    order = np.lexsort((point, rank, node))
    node, point, w = node[order], point[order], w[order]
    s0 = np.zeros(G * G * G)
    np.add.at(s0, node, w)
    s3 = None
    if attr is not None:
        s3 = np.zeros((3, G * G * G))
        for ch in range(3):
            np.add.at(s3[ch], node, w * attr[point, ch])
        s3 = s3.reshape(3, G, G, G)
    return s0.reshape(G, G, G), s3


def _gather_literal(cell, f, wt, attr, G):
    R = G - 1
    members = {}
    for p in range(len(cell)):
        members.setdefault(tuple(int(v) for v in cell[p]), []).append(p)
    s0 = np.zeros((G, G, G))
    s3 = None if attr is None else np.zeros((3, G, G, G))
    for k in range(G):
        for j in range(G):
            for i in range(G):
                acc = [0.0, 0.0, 0.0, 0.0]
                for oz in (-1, 0):
                    for oy in (-1, 0):
                        for ox in (-1, 0):
                            c = (i + ox, j + oy, k + oz)
                            if min(c) < 0 or max(c) >= R:
                                continue
                            for p in members.get(c, ()):
                                fx, fy, fz = (float(v) for v in f[p])
                                wx = fx if ox else 1.0 - fx
                                wy = fy if oy else 1.0 - fy
                                wz = fz if oz else 1.0 - fz
                                w = ((wx * wy) * wz) * float(wt[p])
                                acc[0] += w
                                if attr is not None:
                                    for ch in range(3):
                                        acc[1 + ch] += w * float(attr[p, ch])
                s0[k, j, i] = acc[0]
                if attr is not None:
                    s3[:, k, j, i] = acc[1:]
    return s0, s3


def _density(cell, f, W0):
    dens = np.zeros(len(cell))
    for dz in range(2):
        for dy in range(2):
            for dx in range(2):
                dens = dens + _corner_weight(f, (dx, dy, dz)) * W0[cell[:, 2] + dz, cell[:, 1] + dy, cell[:, 0] + dx]
    return dens


def _density_literal(cell, f, W0):
    dens = np.zeros(len(cell))
    for p in range(len(cell)):
        fx, fy, fz = (float(v) for v in f[p])
        cx, cy, cz = (int(v) for v in cell[p])
        d = 0.0
        for dz in range(2):
            for dy in range(2):
                for dx in range(2):
                    w = ((fx if dx else 1.0 - fx) * (fy if dy else 1.0 - fy)) * (fz if dz else 1.0 - fz)
                    d += w * float(W0[cz + dz, cy + dy, cx + dx])
        dens[p] = d
    return dens


def splat(points, normals, colors, depth, scale, literal=False):
    """-> dict org, h, R, G, W0, C0 (None without colours), dens [n], V (3,G,G,G), D"""
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    nrm = np.asarray(normals, dtype=np.float64).reshape(-1, 3)
    col = None if colors is None else np.asarray(colors, dtype=np.float64).reshape(-1, 3)
    org, h, R, G = grid(pts, depth, scale)
    cell, f = cells(pts, org, h, R)
    gather, density = (_gather_literal, _density_literal) if literal else (_gather, _density)
    W0, C0 = gather(cell, f, np.ones(len(pts)), col, G)
    dens = density(cell, f, W0)
    D, V = gather(cell, f, 1.0 / dens, nrm, G)
    return dict(org=org, h=h, R=R, G=G, W0=W0, C0=C0, dens=dens, V=V, D=D)


# ---- right-hand side ------------------------------------------------------------------------------------------------------------------
def rhs(V):
    """b = -1/2 [(Vx(i+1) - Vx(i-1)) + (Vy(j+1) - Vy(j-1)) + (Vz(k+1) - Vz(k-1))], V zero outside the grid"""
    P = np.pad(V, ((0, 0), (1, 1), (1, 1), (1, 1)))
    dx = P[0, 1:-1, 1:-1, 2:] - P[0, 1:-1, 1:-1, :-2]
    dy = P[1, 1:-1, 2:, 1:-1] - P[1, 1:-1, :-2, 1:-1]
    dz = P[2, 2:, 1:-1, 1:-1] - P[2, :-2, 1:-1, 1:-1]
    return -0.5 * ((dx + dy) + dz)


def rhs_literal(V):
    G = V.shape[1]

    def at(c, k, j, i):
        return float(V[c, k, j, i]) if 0 <= i < G and 0 <= j < G and 0 <= k < G else 0.0

    b = np.zeros((G, G, G))
    for k in range(G):
        for j in range(G):
            for i in range(G):
                b[k, j, i] = -0.5 * (((at(0, k, j, i + 1) - at(0, k, j, i - 1)) + (at(1, k, j + 1, i) - at(1, k, j - 1, i))) +
                                     (at(2, k + 1, j, i) - at(2, k - 1, j, i)))
    return b


# ---- solver, whole arrays -------------------------------------------------------------------------------------------------------------
_IN = (slice(1, -1),) * 3


def _six(x):
    return ((((x[1:-1, 1:-1, 2:] + x[1:-1, 1:-1, :-2]) + x[1:-1, 2:, 1:-1]) + x[1:-1, :-2, 1:-1]) + x[2:, 1:-1, 1:-1]) + x[:-2, 1:-1, 1:-1]


def sweep(x, b, diag, omega):
    y = np.zeros_like(x)
    c = x[_IN]
    y[_IN] = c + omega * ((b[_IN] + _six(x)) / (6.0 + diag[_IN]) - c)
    return y


def residual(x, b, diag):
    r = np.zeros_like(x)
    c = x[_IN]
    r[_IN] = b[_IN] - ((6.0 * c - _six(x)) + diag[_IN] * c)
    return r


def _restrict_axis(f, axis):
    f = np.moveaxis(f, axis, -1)
    n = f.shape[-1]
    P = np.pad(f, [(0, 0)] * (f.ndim - 1) + [(1, 1)])
    out = (0.25 * P[..., 0:n:2] + 0.5 * P[..., 1:n + 1:2]) + 0.25 * P[..., 2:n + 2:2]
    return np.moveaxis(out, -1, axis)


def restrict(f):
    """full weighting: one-axis passes x, y, z; coarse node I takes fine node 2 I; out-of-grid terms are zero"""
    return _restrict_axis(_restrict_axis(_restrict_axis(f, 2), 1), 0)


def _prolong_axis(e, axis):
    e = np.moveaxis(e, axis, -1)
    m = e.shape[-1]
    out = np.zeros(e.shape[:-1] + (2 * m - 1,))
    out[..., 0::2] = e
    out[..., 1::2] = 0.5 * (e[..., :-1] + e[..., 1:])
    return np.moveaxis(out, -1, axis)


def prolong(e):
    return _prolong_axis(_prolong_axis(_prolong_axis(e, 2), 1), 0)


# ---- solver, node by node -------------------------------------------------------------------------------------------------------------
def _six_at(x, k, j, i):
    return ((((float(x[k, j, i + 1]) + float(x[k, j, i - 1])) + float(x[k, j + 1, i])) + float(x[k, j - 1, i])) + float(x[k + 1, j, i])) + float(x[k - 1, j, i])


def sweep_literal(x, b, diag, omega):
    G = x.shape[0]
    y = np.zeros_like(x)
    for k in range(1, G - 1):
        for j in range(1, G - 1):
            for i in range(1, G - 1):
                c = float(x[k, j, i])
                y[k, j, i] = c + omega * ((float(b[k, j, i]) + _six_at(x, k, j, i)) / (6.0 + float(diag[k, j, i])) - c)
    return y


def residual_literal(x, b, diag):
    G = x.shape[0]
    r = np.zeros_like(x)
    for k in range(1, G - 1):
        for j in range(1, G - 1):
            for i in range(1, G - 1):
                c = float(x[k, j, i])
                r[k, j, i] = float(b[k, j, i]) - ((6.0 * c - _six_at(x, k, j, i)) + float(diag[k, j, i]) * c)
    return r


def restrict_literal(f):
    for axis in (2, 1, 0):
        n = f.shape[axis]
        m = (n - 1) // 2 + 1
        shape = list(f.shape)
        shape[axis] = m
        out = np.zeros(shape)
        for at in np.ndindex(*shape):
            src = list(at)

            def val(q):
                if q < 0 or q >= n:
                    return 0.0
                src[axis] = q
                return float(f[tuple(src)])

            I = at[axis]
            out[at] = (0.25 * val(2 * I - 1) + 0.5 * val(2 * I)) + 0.25 * val(2 * I + 1)
        f = out
    return f


def prolong_literal(e):
    for axis in (2, 1, 0):
        m = e.shape[axis]
        shape = list(e.shape)
        shape[axis] = 2 * m - 1
        out = np.zeros(shape)
        for at in np.ndindex(*shape):
            src = list(at)
            q = at[axis]
            if q % 2 == 0:
                src[axis] = q // 2
                out[at] = e[tuple(src)]
            else:
                src[axis] = q // 2
                a = float(e[tuple(src)])
                src[axis] = q // 2 + 1
                out[at] = 0.5 * (a + float(e[tuple(src)]))
        e = out
    return e


# ---- V-cycles -------------------------------------------------------------------------------------------------------------------------
def _vcycle(x, b, diag, p, ops):
    sw, res, rst, pro = ops
    if x.shape[0] <= 5:
        for _ in range(p["coarse_sweeps"]):
            x = sw(x, b, diag, p["omega"])
        return x
    for _ in range(p["pre"]):
        x = sw(x, b, diag, p["omega"])
    bc = 4.0 * rst(res(x, b, diag))
    dc = 4.0 * rst(diag)
    e = _vcycle(np.zeros_like(bc), bc, dc, p, ops)
    x = x.copy()
    x[_IN] = x[_IN] + pro(e)[_IN]
    for _ in range(p["post"]):
        x = sw(x, b, diag, p["omega"])
    return x


def solve(b, D, p, cycles=None, literal=False, history=None):
    """chi after `cycles` V-cycles (default p["cycles"]) from zero.  history: a list that receives chi after every cycle"""
    ops = (sweep_literal, residual_literal, restrict_literal, prolong_literal) if literal else (sweep, residual, restrict, prolong)
    diag = p["alpha"] * D
    x = np.zeros_like(b)
    for _ in range(p["cycles"] if cycles is None else cycles):
        x = _vcycle(x, b, diag, p, ops)
        if history is not None:
            history.append(x)
    return x


def residual_ratio(chi, b, D, alpha):
    """max |b - A chi| / max |b| over the interior nodes"""
    return float(np.abs(residual(chi, b, alpha * D)[_IN]).max() / np.abs(b[_IN]).max())


# ---- extraction -----------------------------------------------------------------------------------------------------------------------
def _empty(C0):
    return np.zeros((0, 3)), np.zeros(0), (None if C0 is None else np.zeros((0, 3))), np.zeros((0, 3), np.int32)


def extract(chi, W0, C0, org, h, table):
    """marching cubes at iso 0 -> vertices [nv,3], densities [nv], colours [nv,3] or None, triangles int32 [nt,3]"""
    G = chi.shape[0]
    table = np.asarray(table, dtype=np.int64).reshape(256, 16)
    count = (table >= 0).sum(1) // 3
    inside = chi < 0.0
    exists = np.zeros((G, G, G, 3), bool)
    exists[:, :, :-1, 0] = inside[:, :, :-1] != inside[:, :, 1:]
    exists[:, :-1, :, 1] = inside[:, :-1, :] != inside[:, 1:, :]
    exists[:-1, :, :, 2] = inside[:-1, :, :] != inside[1:, :, :]
    vid = np.where(exists, np.cumsum(exists.reshape(-1)).reshape(exists.shape) - 1, -1)
    k, j, i, a = np.nonzero(exists)
    nv = len(k)
    if nv == 0:
        return _empty(C0)
    ku, ju, iu = k + (a == 2), j + (a == 1), i + (a == 0)
    ca, cb = chi[k, j, i], chi[ku, ju, iu]
    t = ca / (ca - cb)
    node = np.stack([i, j, k], 1).astype(np.float64)
    vert = org + h * node
    rows = np.arange(nv)
    vert[rows, a] = org[a] + h * (node[rows, a] + t)
    dens = (1.0 - t) * W0[k, j, i] + t * W0[ku, ju, iu]
    col = None
    if C0 is not None:
        with np.errstate(all="ignore"):
            raw = ((1.0 - t) * C0[:, k, j, i] + t * C0[:, ku, ju, iu]) / dens
        col = np.where(dens != 0.0, raw, 0.0).T.copy()
    cube = np.zeros((G - 1, G - 1, G - 1), np.int64)
    for c, (ox, oy, oz) in enumerate(CORNERS):
        cube |= inside[oz:oz + G - 1, oy:oy + G - 1, ox:ox + G - 1].astype(np.int64) << c
    ck, cj, ci = np.nonzero(count[cube] > 0)
    cb_ = cube[ck, cj, ci]
    E = np.stack([vid[ck + EDGE_SHIFT[e][2], cj + EDGE_SHIFT[e][1], ci + EDGE_SHIFT[e][0], EDGE_AXIS[e]] for e in range(12)])     # [12, cubes]
    parts, keys = [], []
    for q in range(5):
        sel = np.nonzero(count[cb_] > q)[0]
        tr = table[cb_[sel]]
        parts.append(np.stack([E[tr[:, 3 * q], sel], E[tr[:, 3 * q + 2], sel], E[tr[:, 3 * q + 1], sel]], 1))
        keys.append(sel * 5 + q)
    tri = np.concatenate(parts)[np.argsort(np.concatenate(keys), kind="stable")]
    return vert, dens, col, tri.astype(np.int32).reshape(-1, 3)


def extract_literal(chi, W0, C0, org, h, table):
    G = chi.shape[0]
    table = [[int(v) for v in row] for row in np.asarray(table).reshape(256, 16)]
    step = ((0, 0, 1), (0, 1, 0), (1, 0, 0))          # [k, j, i] steps of the axes x, y, z
    vertex_of, vert, dens, col = {}, [], [], []
    for k in range(G):
        for j in range(G):
            for i in range(G):
                for a in range(3):
                    ku, ju, iu = k + step[a][0], j + step[a][1], i + step[a][2]
                    if max(ku, ju, iu) >= G:
                        continue
                    ca, cb = float(chi[k, j, i]), float(chi[ku, ju, iu])
                    if (ca < 0.0) == (cb < 0.0):
                        continue
                    t = ca / (ca - cb)
                    p = [float(org[0]) + h * float(i), float(org[1]) + h * float(j), float(org[2]) + h * float(k)]
                    p[a] = float(org[a]) + h * (float((i, j, k)[a]) + t)
                    d = (1.0 - t) * float(W0[k, j, i]) + t * float(W0[ku, ju, iu])
                    vertex_of[(k, j, i, a)] = len(vert)
                    vert.append(p)
                    dens.append(d)
                    if C0 is not None:
                        col.append([((1.0 - t) * float(C0[ch, k, j, i]) + t * float(C0[ch, ku, ju, iu])) / d if d != 0.0 else 0.0 for ch in range(3)])
    tri = []
    for k in range(G - 1):
        for j in range(G - 1):
            for i in range(G - 1):
                index = 0
                for c, (ox, oy, oz) in enumerate(CORNERS):
                    if float(chi[k + oz, j + oy, i + ox]) < 0.0:
                        index |= 1 << c
                row = table[index]
                for q in range(0, 15, 3):
                    if row[q] < 0:
                        break
                    tri.append([vertex_of[(k + EDGE_SHIFT[e][2], j + EDGE_SHIFT[e][1], i + EDGE_SHIFT[e][0], EDGE_AXIS[e])]
                                for e in (row[q], row[q + 2], row[q + 1])])
    if not vert:
        return _empty(C0)
    return (np.array(vert, dtype=np.float64).reshape(-1, 3), np.array(dens, dtype=np.float64),
            None if C0 is None else np.array(col, dtype=np.float64).reshape(-1, 3), np.array(tri, dtype=np.int32).reshape(-1, 3))


# ---- the whole reconstruction ---------------------------------------------------------------------------------------------------------
def fields(points, normals, colors, p, cycles=None, literal=False, history=None):
    """-> the dict of splat() plus b and chi (after `cycles` V-cycles, default all)"""
    S = splat(points, normals, colors, p["depth"], p["scale"], literal=literal)
    S["b"] = (rhs_literal if literal else rhs)(S["V"])
    S["chi"] = solve(S["b"], S["D"], p, cycles, literal=literal, history=history)
    return S


def reconstruct(points, normals, colors, p, table, literal=False):
    """-> vertices, densities, colours or None, triangles"""
    S = fields(points, normals, colors, p, literal=literal)
    return (extract_literal if literal else extract)(S["chi"], S["W0"], S["C0"], S["org"], S["h"], table)


# ---- test clouds ----------------------------------------------------------------------------------------------------------------------
def sphere_cloud(n, radius=0.7, noise=0.0, seed=0, hemisphere=False, colors=True, lattice=False):
    """points on a sphere (or its upper half, open) with outward normals and colours from the direction; `noise` is the standard
    deviation of a radial offset.  Directions are random, or with lattice=True the Fibonacci lattice: n points a distance of about
    sqrt(4 pi / n) radius apart, so a grid of cell size h sees every surface cell sampled once n >= 4 pi radius^2 / h^2 (a random
    cloud of that size leaves exp(-1) of them empty, and the density-normalised normal field is then noise of order one)."""
    rng = np.random.default_rng(seed)
    if lattice:
        i = np.arange(n) + 0.5
        phi, theta = np.arccos(1.0 - 2.0 * i / n), np.pi * (1.0 + 5.0 ** 0.5) * i
        d = np.stack([np.cos(theta) * np.sin(phi), np.sin(theta) * np.sin(phi), np.cos(phi)], 1)
    else:
        d = rng.standard_normal((n, 3))
        d /= np.linalg.norm(d, axis=1)[:, None]
    if hemisphere:
        d[:, 2] = np.abs(d[:, 2])
    pts = d * (radius + noise * rng.standard_normal((n, 1)))
    return pts, d.copy(), (0.5 + 0.5 * d if colors else None)
