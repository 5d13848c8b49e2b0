"""o3d.geometry.TriangleMesh.create_from_point_cloud_poisson on the device ("Poisson reconstruction"; C ABI:
r3d_poisson_*): the screened Poisson formulation on a dense 2^depth grid, float64, every sum in a fixed order.  Parity with Open3D's
octree solver is UNPINNED; tests/poisson_ref.py restates the contract and the device result equals it bit for bit."""
import ctypes

import numpy as np

from . import _lib
from .pointcloud import TriangleMesh, as_arrays

_vp, _i32, _i64, _dbl = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_double
_i64p = ctypes.POINTER(ctypes.c_int64)


class PoissonParams(ctypes.Structure):
    """r3d_poisson_params"""
    _fields_ = [(n, _i32) for n in ("depth", "cycles", "pre", "post", "coarse_sweeps", "reserved")] + [(n, _dbl) for n in ("scale", "alpha", "omega")]


_pp = ctypes.POINTER(PoissonParams)
_reconstruct_sig = ([_vp, _vp, _vp, _vp, _i64, _pp, _i64, _i64, _vp, _vp, _vp, _vp, _i64p, _i64p], ctypes.c_int)
_lib.register({
    "r3d_poisson_reconstruct": _reconstruct_sig,
    "r3d_poisson_reconstruct_dev": _reconstruct_sig,
    "r3d_debug_poisson_fields": ([_vp, _vp, _vp, _vp, _i64, _pp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp], ctypes.c_int),
    "r3d_debug_poisson_extract": ([_vp, _i32, _vp, _dbl, _vp, _vp, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _i64p, _i64p], ctypes.c_int),
})


def poisson_params(depth=8, cycles=10, pre=2, post=2, coarse_sweeps=40, scale=1.1, alpha=4.0, omega=0.8):
    return PoissonParams(int(depth), int(cycles), int(pre), int(post), int(coarse_sweeps), 0, float(scale), float(alpha), float(omega))


_ptr = _lib.ptr


def _rows(a, n=None, name="array"):
    if a is None:
        return None
    a = np.ascontiguousarray(a, dtype=np.float64).reshape(-1, 3)
    if n is not None and len(a) != n:
        raise ValueError(f"{name}: {len(a)} rows for {n} points")
    return a


def _mesh_call(ctx, entry, head, colored, guess):
    """The count / capacity protocol of r3d_poisson_reconstruct and r3d_debug_poisson_extract: one call with the capacities
    `guess`, and a second one with the counts the first returned when they did not fit.
    -> vertices, densities, colours or None, triangles"""
    nv, nt = ctypes.c_int64(), ctypes.c_int64()
    cap_v, cap_t = guess
    while True:
        vert, dens, tri = np.empty((cap_v, 3)), np.empty(cap_v), np.empty((cap_t, 3), np.int32)
        col = np.empty((cap_v, 3)) if colored else None
        rc = getattr(ctx._lib, entry)(ctx._h, *head, cap_v, cap_t, _ptr(vert), _ptr(dens), _ptr(col), _ptr(tri), ctypes.byref(nv), ctypes.byref(nt))
        if rc == _lib.R3D_OK and (nv.value <= cap_v and nt.value <= cap_t):
            break
        if rc == -1 and (nv.value > cap_v or nt.value > cap_t):     # R3D_E_BADARG with the counts: they did not fit
            cap_v, cap_t = nv.value, nt.value
            continue
        ctx.check(rc)
    return vert[:nv.value].copy(), dens[:nv.value].copy(), (col[:nv.value].copy() if colored else None), tri[:nt.value].copy()


def reconstruct(points, normals, colors=None, params=None, ctx=None):
    """r3d_poisson_reconstruct on arrays -> vertices float64 [nv,3], densities float64 [nv], colours float64 [nv,3] or None,
    triangles int32 [nt,3]"""
    ctx = ctx or _lib.default_context()
    prm = params or poisson_params()
    pts = _rows(points)
    nrm, col = _rows(normals, len(pts), "normals"), _rows(colors, len(pts), "colors")
    R = 1 << max(0, min(int(prm.depth), 8))
    head = (_ptr(pts), _ptr(nrm), _ptr(col), len(pts), ctypes.byref(prm))
    return _mesh_call(ctx, "r3d_poisson_reconstruct", head, col is not None, (16 * R * R + 1024, 32 * R * R + 2048))


def reconstruct_device(d_points, d_normals, d_colors, n, params, cap_vertices, cap_triangles, d_vertices, d_densities, d_vertex_colors, d_triangles,
                       ctx=None):
    """r3d_poisson_reconstruct_dev: device pointers (int) in and out -> (vertices, triangles) counted; rows are written when both
    capacities suffice (both 0: the counts alone), else R3DError"""
    ctx = ctx or _lib.default_context()
    nv, nt = ctypes.c_int64(), ctypes.c_int64()
    ctx.call("r3d_poisson_reconstruct_dev", _vp(d_points), _vp(d_normals), _vp(d_colors), int(n), ctypes.byref(params), int(cap_vertices),
             int(cap_triangles), _vp(d_vertices), _vp(d_densities), _vp(d_vertex_colors), _vp(d_triangles), ctypes.byref(nv), ctypes.byref(nt))
    return nv.value, nt.value


def debug_fields(points, normals, colors=None, params=None, k_cycles=None, ctx=None):
    """r3d_debug_poisson_fields -> dict org [3], h, G, W0, D, b, chi (G,G,G) indexed [k,j,i]; C0 (None without colours), V (3,G,G,G);
    dens [n]; chi after k_cycles V-cycles (default: all)"""
    ctx = ctx or _lib.default_context()
    prm = params or poisson_params()
    pts = _rows(points)
    nrm, col = _rows(normals, len(pts), "normals"), _rows(colors, len(pts), "colors")
    G = (1 << max(0, min(int(prm.depth), 8))) + 1
    grid = np.zeros(4)
    out = {n: np.full((G, G, G), np.nan) for n in ("W0", "D", "b", "chi")}
    out["V"] = np.full((3, G, G, G), np.nan)
    out["C0"] = np.full((3, G, G, G), np.nan) if col is not None else None
    out["dens"] = np.full(len(pts), np.nan)
    ctx.call("r3d_debug_poisson_fields", _ptr(pts), _ptr(nrm), _ptr(col), len(pts), ctypes.byref(prm), int(prm.cycles if k_cycles is None else k_cycles),
             _ptr(grid), _ptr(out["W0"]), _ptr(out["C0"]), _ptr(out["dens"]), _ptr(out["V"]), _ptr(out["D"]), _ptr(out["b"]), _ptr(out["chi"]))
    out.update(org=grid[:3].copy(), h=float(grid[3]), G=G)
    return out


def debug_extract(chi, W0, C0, org, h, ctx=None, capacities=None):
    """r3d_debug_poisson_extract: marching cubes at iso 0 on fields of shape (G,G,G) [and (3,G,G,G)], G = 2^depth + 1
    -> vertices, densities, colours or None, triangles"""
    ctx = ctx or _lib.default_context()
    chi = np.ascontiguousarray(chi, dtype=np.float64)
    G = chi.shape[0]
    depth = int(G - 1).bit_length() - 1
    if chi.shape != (G, G, G) or (1 << depth) + 1 != G:
        raise ValueError(f"chi has shape {chi.shape}: expected (G, G, G) with G = 2^depth + 1")
    W0 = np.ascontiguousarray(W0, dtype=np.float64).reshape(G, G, G)
    C0 = None if C0 is None else np.ascontiguousarray(C0, dtype=np.float64).reshape(3, G, G, G)
    org = np.ascontiguousarray(org, dtype=np.float64).reshape(3)
    head = (depth, _ptr(org), float(h), _ptr(chi), _ptr(W0), _ptr(C0))
    return _mesh_call(ctx, "r3d_debug_poisson_extract", head, C0 is not None, capacities or (4096, 8192))


def create_from_point_cloud_poisson(pcd, depth=8, width=0, scale=1.1, linear_fit=False, n_threads=-1, cycles=10, alpha=4.0, ctx=None):
    """TriangleMesh.create_from_point_cloud_poisson(pcd, depth, width, scale, linear_fit, n_threads) -> (TriangleMesh, densities).
    pcd: anything with .points and .normals (and .colors).  The densities are samples per cell at every vertex (Open3D's are a
    log-depth measure): `mesh.remove_vertices_by_mask(densities < np.quantile(densities, q))` trims the same way.  width != 0 and
    linear_fit=True are not built and raise; n_threads is ignored; cycles and alpha are this solver's (V-cycles, screening weight)."""
    if width != 0:
        raise _lib.R3DError(-4, f"create_from_point_cloud_poisson: width={width} is not supported (the grid is set by depth)")
    if linear_fit:
        raise _lib.R3DError(-4, "create_from_point_cloud_poisson: linear_fit=True is not supported")
    pts, col, nrm = as_arrays(pcd)
    if nrm is None:
        raise _lib.R3DError(-1, "create_from_point_cloud_poisson: the point cloud has no normals")
    vert, dens, vcol, tri = reconstruct(pts, nrm, col, poisson_params(depth=depth, cycles=cycles, scale=scale, alpha=alpha), ctx=ctx)
    return TriangleMesh(vert, tri, vcol), dens
