"""Triangle-mesh operations on the device, arrays in and out ("Triangle-mesh operations" and "Mesh topology";
C ABI: r3d_trimesh_*, r3d_meshtopo_*): incidence and adjacency lists, the smoothing filters, normals and the clean-ups; the edge
table, connected components and the welds of duplicated vertices and triangles.  TriangleMesh's methods call these;
mesh_reconstruction.py:22-37 and check84.py:315-322 are what they replace."""
import ctypes
import enum

import numpy as np

from . import _lib

_vp, _i32, _i64, _dbl = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_double
_i64p = ctypes.POINTER(ctypes.c_int64)

SMOOTH_SIMPLE, SMOOTH_LAPLACIAN, SMOOTH_TAUBIN = 0, 1, 2
NORMALS_RAW = 1
DROP_DEGENERATE, DROP_UNREFERENCED, DROP_NON_FINITE = 1, 2, 4
DEDUP_VERTICES, DEDUP_TRIANGLES = 1, 2


class FilterScope(enum.IntEnum):
    """open3d.geometry.FilterScope: which attributes a smoothing filter changes; the others are copied"""
    All = 0
    Color = 1
    Normal = 2
    Vertex = 3


_lists_sig = ([_vp, _i64, _i64, _vp, _i64, _vp, _vp, _i64p], ctypes.c_int)
_smooth_sig = ([_vp, _i64, _i64, _vp, _vp, _vp, _vp, _i32, _i32, _dbl, _dbl, _i32, _vp, _vp, _vp], ctypes.c_int)
_normals_sig = ([_vp, _i64, _i64, _vp, _vp, _i32, _vp, _vp], ctypes.c_int)
_compact_sig = ([_vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i64, _i64, _vp, _vp, _vp, _vp, _i64p, _i64p], ctypes.c_int)
_lib.register({
    "r3d_trimesh_incidence": _lists_sig,
    "r3d_trimesh_adjacency": _lists_sig,
    "r3d_trimesh_smooth": _smooth_sig,
    "r3d_trimesh_smooth_dev": _smooth_sig,
    "r3d_trimesh_normals": _normals_sig,
    "r3d_trimesh_normals_dev": _normals_sig,
    "r3d_trimesh_compact": _compact_sig,
    "r3d_trimesh_compact_dev": _compact_sig,
})


_ptr = _lib.ptr


def _rows(a, n=None, name="array"):
    """float64 [n,3], contiguous; None stays None"""
    if a is None:
        return None
    a = np.ascontiguousarray(a, dtype=np.float64).reshape(-1, 3)
    if n is not None and len(a) != n:
        raise ValueError(f"{name}: {len(a)} rows for {n} vertices")
    return a


def _tri(triangles):
    return np.ascontiguousarray(triangles, dtype=np.int32).reshape(-1, 3)


def _mask(m, n, name):
    if m is None:
        return None
    m = np.ascontiguousarray(np.asarray(m).reshape(-1) != 0, dtype=np.uint8)
    if len(m) != n:
        raise ValueError(f"{name}: {len(m)} entries for {n} rows")
    return m


def _mesh_rows(kv, kt, nrm, col):
    """empty output arrays of a clean-up in the entry points' order: vertices, normals and colours (None where the input has none), triangles"""
    return (np.empty((kv, 3)), np.empty((kv, 3)) if nrm is not None else None, np.empty((kv, 3)) if col is not None else None,
            np.empty((kt, 3), np.int32))


def _lists(entry, n_vertices, triangles, ctx):
    ctx = ctx or _lib.default_context()
    tri = _tri(triangles)
    nv = int(n_vertices)
    return ctx.count_then_fill(entry, (nv, len(tri), _ptr(tri)), 2, lambda n: (np.zeros(nv + 1, np.int32), np.empty(n, np.int32)))[1]


def incidence(n_vertices, triangles, ctx=None):
    """-> offsets int32 [nv + 1], corners int32: vertex v is corner 3 t + c of the triangles listed in corners[offsets[v]:offsets[v + 1]],
    ascending"""
    return _lists("r3d_trimesh_incidence", n_vertices, triangles, ctx)


def adjacency(n_vertices, triangles, ctx=None):
    """-> offsets int32 [nv + 1], neighbours int32: the vertices that share a triangle with v, once each, ascending"""
    return _lists("r3d_trimesh_adjacency", n_vertices, triangles, ctx)


def smooth(vertices, triangles, kind, iterations, lambda_filter=0.5, mu=-0.53, scope=FilterScope.All, normals=None, colors=None, ctx=None):
    """kind: SMOOTH_SIMPLE / SMOOTH_LAPLACIAN / SMOOTH_TAUBIN -> (vertices, normals or None, colours or None), new arrays"""
    ctx = ctx or _lib.default_context()
    if int(iterations) < 0:
        raise ValueError(f"number_of_iterations must not be negative (got {iterations})")
    vert, tri = _rows(vertices), _tri(triangles)
    nv = len(vert)
    nrm, col = _rows(normals, nv, "normals"), _rows(colors, nv, "colors")
    out = [np.empty_like(a) if a is not None else None for a in (vert, nrm, col)]
    ctx.call("r3d_trimesh_smooth", nv, len(tri), _ptr(vert), _ptr(nrm), _ptr(col), _ptr(tri), int(kind), int(iterations), float(lambda_filter), float(mu),
             int(scope), _ptr(out[0]), _ptr(out[1]), _ptr(out[2]))
    return tuple(out)


def smooth_device(d_vertices, d_triangles, n_vertices, n_triangles, kind, iterations, d_out_vertices, lambda_filter=0.5, mu=-0.53,
                  scope=FilterScope.All, d_normals=None, d_colors=None, d_out_normals=None, d_out_colors=None, ctx=None):
    """r3d_trimesh_smooth_dev: device pointers (int) in and out, e.g. the arrays extract_mesh_device wrote"""
    ctx = ctx or _lib.default_context()
    ctx.call("r3d_trimesh_smooth_dev", int(n_vertices), int(n_triangles), _vp(d_vertices), _vp(d_normals), _vp(d_colors), _vp(d_triangles), int(kind),
             int(iterations), float(lambda_filter), float(mu), int(scope), _vp(d_out_vertices), _vp(d_out_normals), _vp(d_out_colors))


def triangle_normals(vertices, triangles, raw=False, ctx=None):
    """(v1 - v0) x (v2 - v0) per triangle, normalised unless raw; a zero vector stays zero"""
    ctx = ctx or _lib.default_context()
    vert, tri = _rows(vertices), _tri(triangles)
    out = np.empty((len(tri), 3))
    ctx.call("r3d_trimesh_normals", len(vert), len(tri), _ptr(vert), _ptr(tri), NORMALS_RAW if raw else 0, _ptr(out), None)
    return out


def vertex_normals(vertices, triangles, raw=False, ctx=None):
    """the unnormalised cross products of a vertex's triangles added in ascending corner order, normalised unless raw"""
    ctx = ctx or _lib.default_context()
    vert, tri = _rows(vertices), _tri(triangles)
    out = np.empty((len(vert), 3))
    ctx.call("r3d_trimesh_normals", len(vert), len(tri), _ptr(vert), _ptr(tri), NORMALS_RAW if raw else 0, None, _ptr(out))
    return out


def normals_device(d_vertices, d_triangles, n_vertices, n_triangles, d_triangle_normals=None, d_vertex_normals=None, raw=False, ctx=None):
    """r3d_trimesh_normals_dev: device pointers (int); either output may be None"""
    ctx = ctx or _lib.default_context()
    ctx.call("r3d_trimesh_normals_dev", int(n_vertices), int(n_triangles), _vp(d_vertices), _vp(d_triangles), NORMALS_RAW if raw else 0,
             _vp(d_triangle_normals), _vp(d_vertex_normals))


def compact_counts(vertices, triangles, flags=0, vertex_keep=None, triangle_keep=None, ctx=None):
    """-> (vertices, triangles) that compact() would keep"""
    ctx = ctx or _lib.default_context()
    vert, tri = _rows(vertices), _tri(triangles)
    vk, tk = _mask(vertex_keep, len(vert), "vertex_keep"), _mask(triangle_keep, len(tri), "triangle_keep")
    nv, nt = ctypes.c_int64(), ctypes.c_int64()
    ctx.call("r3d_trimesh_compact", len(vert), len(tri), _ptr(vert), None, None, _ptr(tri), _ptr(vk), _ptr(tk), int(flags), 0, 0, None, None, None, None,
             ctypes.byref(nv), ctypes.byref(nt))
    return nv.value, nt.value


def compact(vertices, triangles, flags=0, vertex_keep=None, triangle_keep=None, normals=None, colors=None, ctx=None):
    """The clean-ups in one call.  flags: DROP_DEGENERATE | DROP_UNREFERENCED | DROP_NON_FINITE; the keep masks are truthy where a
    row stays.  Triangles are decided first; survivors keep their order.  -> (vertices, triangles, normals or None, colours or None)"""
    ctx = ctx or _lib.default_context()
    vert, tri = _rows(vertices), _tri(triangles)
    nv, nt = len(vert), len(tri)
    nrm, col = _rows(normals, nv, "normals"), _rows(colors, nv, "colors")
    vk, tk = _mask(vertex_keep, nv, "vertex_keep"), _mask(triangle_keep, nt, "triangle_keep")
    args = (nv, nt, _ptr(vert), _ptr(nrm), _ptr(col), _ptr(tri), _ptr(vk), _ptr(tk), int(flags))
    _, (ov, on, oc, ot) = ctx.count_then_fill("r3d_trimesh_compact", args, 4, lambda kv, kt: _mesh_rows(kv, kt, nrm, col), n_counts=2)
    return ov, ot, on, oc


def compact_device(d_vertices, d_triangles, n_vertices, n_triangles, flags, cap_vertices, cap_triangles, d_out_vertices, d_out_triangles,
                   d_vertex_keep=None, d_triangle_keep=None, d_normals=None, d_colors=None, d_out_normals=None, d_out_colors=None, ctx=None):
    """r3d_trimesh_compact_dev: device pointers (int) -> the numbers of vertex and triangle rows kept (written when both fit)"""
    ctx = ctx or _lib.default_context()
    kv, kt = ctypes.c_int64(), ctypes.c_int64()
    ctx.call("r3d_trimesh_compact_dev", int(n_vertices), int(n_triangles), _vp(d_vertices), _vp(d_normals), _vp(d_colors), _vp(d_triangles),
             _vp(d_vertex_keep), _vp(d_triangle_keep), int(flags), int(cap_vertices), int(cap_triangles), _vp(d_out_vertices), _vp(d_out_normals),
             _vp(d_out_colors), _vp(d_out_triangles), ctypes.byref(kv), ctypes.byref(kt))
    return kv.value, kt.value


# ---- mesh topology (csrc/meshtopo.hip) ------------------------------------------------------------------------------------------------
def sort_pairs_u64(keys, bits=64, values=None, ctx=None):
    """r3d_debug_sort_pairs_u64: -> (keys, values) in the stable order of the keys' low `bits` bits; values default to the index"""
    ctx = ctx or _lib.default_context()
    keys = np.ascontiguousarray(keys, dtype=np.uint64).reshape(-1)
    vals = None if values is None else np.ascontiguousarray(values, dtype=np.int32).reshape(-1)
    if vals is not None and len(vals) != len(keys):
        raise ValueError(f"{len(vals)} values for {len(keys)} keys")
    ok, ov = np.empty_like(keys), np.empty(len(keys), np.int32)
    ctx.call("r3d_debug_sort_pairs_u64", _ptr(keys), _ptr(vals), len(keys), int(bits), _ptr(ok), _ptr(ov))
    return ok, ov


def edges(n_vertices, triangles, ctx=None):
    """-> edges int32 [n,2] (min, max) ascending, counts int32 [n] (sides on each), stats int64 [4] = (edges, boundary, non-manifold,
    degenerate)"""
    ctx = ctx or _lib.default_context()
    tri = _tri(triangles)
    nv, nt = int(n_vertices), len(tri)
    n, stats = ctypes.c_int64(), np.zeros(4, np.int64)
    ctx.call("r3d_meshtopo_edges", nv, nt, _ptr(tri), 0, None, None, _ptr(stats), ctypes.byref(n))
    edg, cnt = np.empty((n.value, 2), np.int32), np.empty(n.value, np.int32)
    if n.value:
        got = ctypes.c_int64()
        ctx.call("r3d_meshtopo_edges", nv, nt, _ptr(tri), n.value, _ptr(edg), _ptr(cnt), _ptr(stats), ctypes.byref(got))
        assert got.value == n.value
    return edg, cnt, stats


def components(vertices, triangles, ctx=None):
    """cluster_connected_triangles -> triangle_clusters int32 [nt] (components in ascending order of their lowest triangle),
    cluster_n_triangles int64 [], cluster_area float64 []"""
    ctx = ctx or _lib.default_context()
    vert, tri = _rows(vertices), _tri(triangles)
    nv, nt = len(vert), len(tri)
    labels, n = np.empty(nt, np.int32), ctypes.c_int64()
    ctx.call("r3d_meshtopo_components", nv, nt, _ptr(vert), _ptr(tri), 0, _ptr(labels), None, None, ctypes.byref(n))
    cnt, area = np.empty(n.value, np.int64), np.empty(n.value, np.float64)
    if n.value:
        got = ctypes.c_int64()
        ctx.call("r3d_meshtopo_components", nv, nt, _ptr(vert), _ptr(tri), n.value, _ptr(labels), _ptr(cnt), _ptr(area), ctypes.byref(got))
        assert got.value == n.value
    return labels, cnt, area


def components_device(d_vertices, d_triangles, n_vertices, n_triangles, d_triangle_clusters, cap_clusters=0, d_cluster_n_triangles=None,
                      d_cluster_area=None, ctx=None):
    """r3d_meshtopo_components_dev: device pointers (int) -> the number of clusters; counts and areas are written when they fit"""
    ctx = ctx or _lib.default_context()
    n = ctypes.c_int64()
    ctx.call("r3d_meshtopo_components_dev", int(n_vertices), int(n_triangles), _vp(d_vertices), _vp(d_triangles), int(cap_clusters),
             _vp(d_triangle_clusters), _vp(d_cluster_n_triangles), _vp(d_cluster_area), ctypes.byref(n))
    return n.value


def dedup(vertices, triangles, flags=DEDUP_VERTICES | DEDUP_TRIANGLES, normals=None, colors=None, ctx=None):
    """The welds.  flags: DEDUP_VERTICES | DEDUP_TRIANGLES (vertices first).  The first occurrence survives; survivors keep their
    order.  -> (vertices, triangles, normals or None, colours or None, vertex_map int32 [nv], triangle_origin int32 [out nt])"""
    ctx = ctx or _lib.default_context()
    vert, tri = _rows(vertices), _tri(triangles)
    nv, nt = len(vert), len(tri)
    nrm, col = _rows(normals, nv, "normals"), _rows(colors, nv, "colors")
    args = (nv, nt, _ptr(vert), _ptr(nrm), _ptr(col), _ptr(tri), int(flags))

    def outputs(kv, kt):
        return _mesh_rows(kv, kt, nrm, col) + (np.empty(nv, np.int32), np.empty(kt, np.int32))

    _, (ov, on, oc, ot, vmap, origin) = ctx.count_then_fill("r3d_meshtopo_dedup", args, 6, outputs, n_counts=2)
    return ov, ot, on, oc, vmap, origin


def dedup_device(d_vertices, d_triangles, n_vertices, n_triangles, flags, cap_vertices, cap_triangles, d_out_vertices, d_out_triangles,
                 d_normals=None, d_colors=None, d_out_normals=None, d_out_colors=None, d_vertex_map=None, d_triangle_origin=None, ctx=None):
    """r3d_meshtopo_dedup_dev: device pointers (int) -> the numbers of vertex and triangle rows kept (written when both fit)"""
    ctx = ctx or _lib.default_context()
    kv, kt = ctypes.c_int64(), ctypes.c_int64()
    ctx.call("r3d_meshtopo_dedup_dev", int(n_vertices), int(n_triangles), _vp(d_vertices), _vp(d_normals), _vp(d_colors), _vp(d_triangles), int(flags),
             int(cap_vertices), int(cap_triangles), _vp(d_out_vertices), _vp(d_out_normals), _vp(d_out_colors), _vp(d_out_triangles), _vp(d_vertex_map),
             _vp(d_triangle_origin), ctypes.byref(kv), ctypes.byref(kt))
    return kv.value, kt.value


def component_mask(labels, n_triangles, areas, min_triangles=0, min_area=0.0, keep_largest=False):
    """The tutorial idiom on the arrays of components(), in numpy: -> bool [nt], True where a triangle is to be REMOVED.  A component
    goes when it has fewer than min_triangles triangles or less than min_area area; keep_largest removes every component but the
    one with the most triangles (ties: the lower label)."""
    labels = np.asarray(labels).reshape(-1)
    n_triangles, areas = np.asarray(n_triangles).reshape(-1), np.asarray(areas, dtype=np.float64).reshape(-1)
    if len(n_triangles) != len(areas):
        raise ValueError(f"{len(n_triangles)} triangle counts for {len(areas)} areas")
    drop = (n_triangles < min_triangles) | (areas < min_area)
    if keep_largest and len(n_triangles):
        only = np.ones(len(n_triangles), bool)
        only[int(np.argmax(n_triangles))] = False         # argmax returns the first of equals
        drop |= only
    return drop[labels] if len(labels) else np.zeros(0, bool)
