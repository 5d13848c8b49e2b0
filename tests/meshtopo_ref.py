"""The mesh-topology contract ("Mesh topology") restated twice, like tests/trimesh_ref.py: a literal form (dicts,
a breadth-first search from the first unvisited triangle, Python loops) and a vectorised numpy form, which tests/test_meshtopo_ref.py
holds equal on the CPU and tests/test_meshtopo_gpu.py compares the device against bit for bit.

Recalled from Open3D 0.18 TriangleMesh.cpp; parity with Open3D is unpinned.  What memory leaves open is a named switch here."""
import numpy as np

EDGE_ORDER = "ascending (min, max)"     # Open3D keeps a hash map whose order is unspecified
AREA_CHUNK = 256                        # cluster_area: chunks of this many terms from the front, then the chunk sums from the front
NAN_EQUALS_NOTHING = True               # remove_duplicated_vertices: a row holding a NaN is never a duplicate, not even of itself
TRIANGLE_KEY = "smallest rotation"      # remove_duplicated_triangles: the lexicographically smallest of the three rotations
DEDUP_VERTICES, DEDUP_TRIANGLES = 1, 2


def _tri(triangles):
    return np.ascontiguousarray(triangles, dtype=np.int64).reshape(-1, 3)


def _bit_length(x):
    return int(x).bit_length() if x > 0 else 0


# ---- edge table ------------------------------------------------------------------------------------------------------------------------
def sorted_sides(nv, triangles):
    """-> keys uint64 [3m] ascending ((min << b) | max, b the bit length of nv - 1), the side 3 t + c of each (stable), b"""
    t = _tri(triangles)
    if len(t) and (t.min() < 0 or t.max() >= nv):
        raise ValueError(f"a triangle index outside [0, {nv})")
    p, q = t.reshape(-1), t[:, [1, 2, 0]].reshape(-1)
    b = _bit_length(nv - 1)
    key = (np.minimum(p, q).astype(np.uint64) << np.uint64(b)) | np.maximum(p, q).astype(np.uint64)
    order = np.argsort(key, kind="stable")
    return key[order], order, b


def edges(nv, triangles):
    """-> edges int32 [n,2], counts int32 [n], stats int64 [4] = (edges, boundary, non-manifold, degenerate)"""
    key, _, b = sorted_sides(nv, triangles)
    if not len(key):
        return np.zeros((0, 2), np.int32), np.zeros(0, np.int32), np.zeros(4, np.int64)
    head = np.flatnonzero(np.concatenate([[True], key[1:] != key[:-1]]))
    counts = np.diff(np.concatenate([head, [len(key)]])).astype(np.int32)
    k = key[head]
    edg = np.stack([k >> np.uint64(b), k & np.uint64((1 << b) - 1)], 1).astype(np.int32)
    stats = np.array([len(k), (counts == 1).sum(), (counts > 2).sum(), (edg[:, 0] == edg[:, 1]).sum()], np.int64)
    return edg, counts, stats


def edges_literal(nv, triangles):
    table = {}
    for a, b, c in _tri(triangles).tolist():
        for p, q in ((a, b), (b, c), (c, a)):
            if not (0 <= p < nv and 0 <= q < nv):
                raise ValueError(f"a triangle index outside [0, {nv})")
            e = (min(p, q), max(p, q))
            table[e] = table.get(e, 0) + 1
    keys = sorted(table)
    counts = [table[e] for e in keys]
    stats = [len(keys), sum(c == 1 for c in counts), sum(c > 2 for c in counts), sum(p == q for p, q in keys)]
    return np.array(keys, np.int32).reshape(-1, 2), np.array(counts, np.int32), np.array(stats, np.int64)


def non_manifold_edges(nv, triangles, allow_boundary_edges=True):
    edg, counts, _ = edges(nv, triangles)
    return edg[counts > 2 if allow_boundary_edges else counts != 2]


def euler_poincare_characteristic(nv, triangles):
    return nv + len(_tri(triangles)) - int(edges(nv, triangles)[2][0])


# ---- components ------------------------------------------------------------------------------------------------------------------------
def links(nv, triangles):
    """the pairs of triangles joined by neighbouring sides of one edge in the sorted order: a run of k sides gives k - 1 links"""
    key, side, _ = sorted_sides(nv, triangles)
    if len(key) < 2:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    same = np.flatnonzero(key[1:] == key[:-1]) + 1
    return side[same] // 3, side[same - 1] // 3


def area_terms(vertices, triangles):
    """0.5 * norm(cross(p1 - p0, p2 - p0)) per triangle, every operation written out (float64, no fused multiply-add)"""
    v, t = np.asarray(vertices, dtype=np.float64).reshape(-1, 3), _tri(triangles)
    a, b = v[t[:, 1]] - v[t[:, 0]], v[t[:, 2]] - v[t[:, 0]]
    n0 = a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1]
    n1 = a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2]
    n2 = a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]
    return 0.5 * np.sqrt((n0 * n0 + n1 * n1) + n2 * n2)


def area_sums(terms, labels, n_clusters):
    """per component: its terms in ascending triangle index, consecutive chunks of AREA_CHUNK summed from the front (from 0.0), then
    the chunk sums from the front (from 0.0)"""
    order = np.argsort(labels, kind="stable")
    count = np.bincount(labels, minlength=n_clusters).astype(np.int64)
    chunks = (count + AREA_CHUNK - 1) // AREA_CHUNK
    chunk_start = np.concatenate([[0], np.cumsum(chunks)])
    start = np.concatenate([[0], np.cumsum(count)])
    # every component padded with +0.0 to whole chunks: x + 0.0 is x, so a padded chunk sums to what the short one does
    lab = labels[order]
    slot = chunk_start[lab] * AREA_CHUNK + (np.arange(len(order)) - start[lab])
    padded = np.zeros(int(chunk_start[-1]) * AREA_CHUNK)
    padded[slot] = terms[order]
    csum = np.add.accumulate(padded.reshape(-1, AREA_CHUNK), axis=1)[:, -1] if len(padded) else np.zeros(0)   # accumulate is sequential
    total = np.zeros(n_clusters)
    for r in range(int(chunks.max()) if n_clusters else 0):
        sel = np.flatnonzero(chunks > r)
        total[sel] = total[sel] + csum[chunk_start[sel] + r]
    return total


def components(vertices, triangles, rounds_out=None):
    """-> triangle_clusters int32 [m], cluster_n_triangles int64 [], cluster_area float64 [].  Min-label hooking with pointer jumping:
    every link hooks the larger of its two roots under the smaller, then every parent is replaced by its parent until nothing moves."""
    v, t = np.asarray(vertices, dtype=np.float64).reshape(-1, 3), _tri(triangles)
    nt = len(t)
    a, b = links(len(v), t)
    parent = np.arange(nt)
    rounds = 0
    while True:
        ra, rb = parent[a], parent[b]
        differ = ra != rb
        if not differ.any():
            break
        rounds += 1
        np.minimum.at(parent, np.maximum(ra, rb)[differ], np.minimum(ra, rb)[differ])
        while True:
            nxt = parent[parent]
            if np.array_equal(nxt, parent):
                break
            parent = nxt
    if rounds_out is not None:
        rounds_out.append(rounds)
    is_root = parent == np.arange(nt)
    number = np.cumsum(is_root) - 1             # the components in ascending order of their root, which is their lowest triangle
    labels = number[parent].astype(np.int32)
    ncl = int(is_root.sum())
    count = np.zeros(ncl, np.int64)
    np.add.at(count, labels, 1)
    return labels, count, area_sums(area_terms(v, t), labels.astype(np.int64), ncl)


def components_literal(vertices, triangles):
    """breadth-first search from the first unvisited triangle, as Open3D scans; the areas in the contract's own order"""
    v, t = np.asarray(vertices, dtype=np.float64).reshape(-1, 3), _tri(triangles).tolist()
    on_edge = {}
    for i, (a, b, c) in enumerate(t):
        for p, q in ((a, b), (b, c), (c, a)):
            on_edge.setdefault((min(p, q), max(p, q)), []).append(i)
    labels = [-1] * len(t)
    ncl = 0
    for s in range(len(t)):
        if labels[s] >= 0:
            continue
        labels[s] = ncl
        queue = [s]
        while queue:
            i = queue.pop()
            a, b, c = t[i]
            for p, q in ((a, b), (b, c), (c, a)):
                for j in on_edge[(min(p, q), max(p, q))]:
                    if labels[j] < 0:
                        labels[j] = ncl
                        queue.append(j)
        ncl += 1
    terms = area_terms(v, t).tolist() if len(t) else []
    members = [[] for _ in range(ncl)]
    for i, l in enumerate(labels):
        members[l].append(i)
    areas = []
    for m in members:
        total = 0.0
        for k in range(0, len(m), AREA_CHUNK):
            s = 0.0
            for i in m[k:k + AREA_CHUNK]:
                s += terms[i]
            total += s
        areas.append(total)
    return np.array(labels, np.int32), np.array([len(m) for m in members], np.int64), np.array(areas, np.float64)


# ---- welds -----------------------------------------------------------------------------------------------------------------------------
def _first_of_runs(order, head):
    """first[i]: the lowest index of the run that holds i (order is stable, so that is the run's head)"""
    run = np.cumsum(head) - 1
    first = np.empty(len(order), np.int64)
    first[order] = order[np.flatnonzero(head)][run]
    return first


def vertex_first(vertices):
    """first[v]: the lowest vertex that equals v as three IEEE doubles (-0.0 == +0.0; a row with a NaN equals nothing)"""
    v = np.ascontiguousarray(vertices, dtype=np.float64).reshape(-1, 3)
    if not len(v):
        return np.zeros(0, np.int64)
    folded = (v + 0.0).view(np.uint64)                      # -0.0 + 0.0 is +0.0; every other bit pattern stays
    order = np.lexsort((folded[:, 2], folded[:, 1], folded[:, 0]))      # stable
    s = v[order]
    with np.errstate(invalid="ignore"):
        head = np.concatenate([[True], ~(s[1:] == s[:-1]).all(1)])
    return _first_of_runs(order, head)


def canonical(triangles):
    """each triangle rotated to the lexicographically smallest of its three rotations"""
    t = _tri(triangles)
    best = t.copy()
    for r in (t[:, [1, 2, 0]], t[:, [2, 0, 1]]):
        less = (r[:, 0] < best[:, 0]) | ((r[:, 0] == best[:, 0]) & ((r[:, 1] < best[:, 1]) | ((r[:, 1] == best[:, 1]) & (r[:, 2] < best[:, 2]))))
        best = np.where(less[:, None], r, best)
    return best


def triangle_first(triangles):
    c = canonical(triangles)
    if not len(c):
        return np.zeros(0, np.int64)
    order = np.lexsort((c[:, 2], c[:, 1], c[:, 0]))
    s = c[order]
    head = np.concatenate([[True], (s[1:] != s[:-1]).any(1)])
    return _first_of_runs(order, head)


def dedup(vertices, triangles, flags=DEDUP_VERTICES | DEDUP_TRIANGLES, normals=None, colors=None):
    """-> (vertices, triangles int32, normals or None, colours or None, vertex_map int32 [nv], triangle_origin int32 [out nt])"""
    v, t = np.ascontiguousarray(vertices, dtype=np.float64).reshape(-1, 3), _tri(triangles)
    nv = len(v)
    if len(t) and (t.min() < 0 or t.max() >= nv):
        raise ValueError(f"a triangle index outside [0, {nv})")
    vmap = np.arange(nv)
    keep_v = np.ones(nv, bool)
    if flags & DEDUP_VERTICES:
        first = vertex_first(v)
        keep_v = first == np.arange(nv)
        vmap = (np.cumsum(keep_v) - 1)[first]
        t = vmap[t] if len(t) else t
    origin = np.arange(len(t))
    if flags & DEDUP_TRIANGLES:
        origin = np.flatnonzero(triangle_first(t) == np.arange(len(t)))
    rows = lambda a: None if a is None else np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(-1, 3)[keep_v])     # noqa: E731
    return (np.ascontiguousarray(v[keep_v]), np.ascontiguousarray(t[origin], dtype=np.int32).reshape(-1, 3), rows(normals), rows(colors),
            vmap.astype(np.int32), origin.astype(np.int32))


def dedup_literal(vertices, triangles, flags=DEDUP_VERTICES | DEDUP_TRIANGLES, normals=None, colors=None):
    v, t = np.ascontiguousarray(vertices, dtype=np.float64).reshape(-1, 3), _tri(triangles).tolist()
    nv = len(v)
    kept, vmap = list(range(nv)), list(range(nv))
    if flags & DEDUP_VERTICES:
        seen, kept, vmap = {}, [], []
        for i, row in enumerate(v.tolist()):
            key = tuple(x + 0.0 for x in row)                # -0.0 and +0.0 hash and compare equal anyway
            if any(x != x for x in row) or key not in seen:
                if not any(x != x for x in row):
                    seen[key] = len(kept)
                vmap.append(len(kept))
                kept.append(i)
            else:
                vmap.append(seen[key])
        t = [[vmap[a] for a in row] for row in t]
    origin = list(range(len(t)))
    if flags & DEDUP_TRIANGLES:
        seen, origin = set(), []
        for i, (a, b, c) in enumerate(t):
            key = min((a, b, c), (b, c, a), (c, a, b))
            if key not in seen:
                seen.add(key)
                origin.append(i)
    rows = lambda a: None if a is None else np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(-1, 3)[kept])       # noqa: E731
    return (np.ascontiguousarray(v[kept]), np.array([t[i] for i in origin], np.int32).reshape(-1, 3), rows(normals), rows(colors),
            np.array(vmap, np.int32), np.array(origin, np.int32))


def component_mask(labels, n_triangles, areas, min_triangles=0, min_area=0.0, keep_largest=False):
    """True where a triangle is removed; 'largest' is by triangle count, ties to the lower label"""
    drop = [n < min_triangles or a < min_area for n, a in zip(n_triangles, areas)]
    if keep_largest and len(n_triangles):
        best = max(range(len(n_triangles)), key=lambda c: (n_triangles[c], -c))
        drop = [d or c != best for c, d in enumerate(drop)]
    return np.array([drop[l] for l in labels], bool)
