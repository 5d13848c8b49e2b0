"""Minimal stand-in for open3d.geometry.PointCloud (Open3D is not installed here or on the GPU box).

The drop-in classes accept ANY object exposing .points / .normals / .colors convertible by np.asarray (a real legacy
Open3D cloud works: its Vector3dVector attributes convert and can be assigned back) or this small class.
Mirrors the members the reference uses: `+=` (main.py:49), transform (pointcloud_alignment.py:42), has_normals
(test/GICP1.py:94-97), len(pcd.points) (main.py:39,42).
"""
import numpy as np


def _arr(a):
    if a is None:
        return np.zeros((0, 3))
    a = np.asarray(a, dtype=np.float64)
    return a.reshape(-1, 3) if a.size else np.zeros((0, 3))


class PointCloud:
    def __init__(self, points=None, colors=None, normals=None):
        self.points = _arr(points)
        self.colors = _arr(colors)
        self.normals = _arr(normals)

    def has_points(self):
        return len(self.points) > 0

    def has_normals(self):
        return len(self.normals) > 0 and len(self.normals) == len(self.points)

    def has_colors(self):
        return len(self.colors) > 0 and len(self.colors) == len(self.points)

    def __len__(self):
        return len(self.points)

    def __iadd__(self, other):
        """Legacy operator+=: attributes survive only if BOTH clouds carry them (or self was empty)."""
        n0 = len(self.points)
        op, on, oc = _arr(other.points), _arr(getattr(other, "normals", None)), _arr(getattr(other, "colors", None))
        keep_n = (n0 == 0 or self.has_normals()) and len(on) == len(op) and len(op) > 0
        keep_c = (n0 == 0 or self.has_colors()) and len(oc) == len(op) and len(op) > 0
        self.normals = np.concatenate([_arr(self.normals), on]) if keep_n else np.zeros((0, 3))
        self.colors = np.concatenate([_arr(self.colors), oc]) if keep_c else np.zeros((0, 3))
        self.points = np.concatenate([_arr(self.points), op])
        return self

    def __add__(self, other):
        out = PointCloud(self.points.copy(), self.colors.copy(), self.normals.copy())
        out += other
        return out

    def transform(self, T):
        from . import cloud_ops
        T = np.asarray(T, dtype=np.float64)
        if len(self.points):
            self.points = cloud_ops.transform_points(self.points, T)
        if self.has_normals():
            self.normals = cloud_ops.transform_points(self.normals, T, rotate_only=True)
        return self

    def voxel_down_sample(self, voxel_size):
        from . import cloud_ops
        p, c, n = cloud_ops.voxel_down_sample(self.points, voxel_size, self.colors if self.has_colors() else None,
                                              self.normals if self.has_normals() else None)
        return PointCloud(p, c, n)

    def estimate_normals(self, radius=None, max_nn=30, search_param=None):
        """estimate_normals(search_param=KDTreeSearchParamHybrid(radius, max_nn)) -- pass the two numbers, or any
        object with .radius / .max_nn (or .knn) attributes."""
        from . import cloud_ops
        if search_param is not None:
            radius = getattr(search_param, "radius", None)
            max_nn = getattr(search_param, "max_nn", getattr(search_param, "knn", max_nn))
        self.normals = cloud_ops.estimate_normals(self.points, radius, max_nn,
                                                  self.normals if self.has_normals() else None)
        return self


class TriangleMesh:
    """Minimal stand-in for open3d.geometry.TriangleMesh, what ScalableTSDFVolume.extract_triangle_mesh returns: vertices float64
    [n,3], vertex_colors float64 [n,3] or None, triangles int32 [m,3], vertex_normals float64 [n,3] or None (until
    compute_vertex_normals).  io_formats.write_ply(path, mesh.vertices, colors=mesh.vertex_colors, faces=mesh.triangles) saves it.
    The filters, compute_triangle_normals, compute_adjacency_list, the remove_* clean-ups, cluster_connected_triangles and the edge
    queries run on the device (mesh_ops.py); triangle_normals (float64 [m,3]) and adjacency_list (a list of ascending int32 arrays)
    are None until computed.  mesh_a + mesh_b concatenates, as Open3D's operator+."""

    def __init__(self, vertices=None, triangles=None, vertex_colors=None, vertex_normals=None):
        self.vertices = _arr(vertices)
        self.triangles = np.zeros((0, 3), np.int32) if triangles is None else np.ascontiguousarray(triangles, dtype=np.int32).reshape(-1, 3)
        self.vertex_colors = None if vertex_colors is None else _arr(vertex_colors)
        self.vertex_normals = None if vertex_normals is None else _arr(vertex_normals)
        self.triangle_normals = None
        self.adjacency_list = None

    @staticmethod
    def create_from_point_cloud_poisson(pcd, depth=8, width=0, scale=1.1, linear_fit=False, n_threads=-1, **solver):
        """-> (TriangleMesh, densities): poisson.create_from_point_cloud_poisson, on the device"""
        from . import poisson
        return poisson.create_from_point_cloud_poisson(pcd, depth, width, scale, linear_fit, n_threads, **solver)

    def has_vertices(self):
        return len(self.vertices) > 0

    def has_triangles(self):
        return len(self.vertices) > 0 and len(self.triangles) > 0

    def has_vertex_colors(self):
        return self.vertex_colors is not None and len(self.vertices) > 0 and len(self.vertex_colors) == len(self.vertices)

    def has_vertex_normals(self):
        return self.vertex_normals is not None and len(self.vertices) > 0 and len(self.vertex_normals) == len(self.vertices)

    def compute_vertex_normals(self, device=False, ctx=None):
        """Open3D's scheme [recalled]: every triangle adds its unnormalised cross product (v1 - v0) x (v2 - v0) to its three
        vertices, in triangle order; the sums are normalised, a zero sum stays zero.  On the host in numpy: a helper.
        device=True: the same sums in the same order on the device (mesh_ops.vertex_normals), bit for bit."""
        if device:
            from . import mesh_ops
            self.vertex_normals = mesh_ops.vertex_normals(self.vertices, self.triangles, ctx=ctx)
            return self
        v, t = self.vertices, self.triangles
        normals = np.zeros((len(v), 3))
        if len(t):
            face = np.cross(v[t[:, 1]] - v[t[:, 0]], v[t[:, 2]] - v[t[:, 0]])
            np.add.at(normals, t.reshape(-1), np.repeat(face, 3, axis=0))       # unbuffered: a vertex's sum runs in triangle order
        length = np.sqrt((normals * normals).sum(1))
        with np.errstate(all="ignore"):
            self.vertex_normals = np.where(length[:, None] != 0, normals / length[:, None], normals)
        return self

    def has_triangle_normals(self):
        return self.triangle_normals is not None and len(self.triangles) > 0 and len(self.triangle_normals) == len(self.triangles)

    def has_adjacency_list(self):
        return self.adjacency_list is not None and len(self.vertices) > 0 and len(self.adjacency_list) == len(self.vertices)

    def compute_triangle_normals(self, ctx=None):
        """(v1 - v0) x (v2 - v0) per triangle, normalised; a zero vector stays zero"""
        from . import mesh_ops
        self.triangle_normals = mesh_ops.triangle_normals(self.vertices, self.triangles, ctx=ctx)
        return self

    def compute_adjacency_list(self, ctx=None):
        """adjacency_list[v]: the vertices that share a triangle with v, ascending (Open3D keeps unordered sets)"""
        from . import mesh_ops
        off, nb = mesh_ops.adjacency(len(self.vertices), self.triangles, ctx=ctx)
        self.adjacency_list = [nb[off[v]:off[v + 1]] for v in range(len(self.vertices))]
        return self

    # ---- smoothing filters: a new mesh, as in Open3D; triangles unchanged, unfiltered attributes copied
    def _filtered(self, kind, number_of_iterations, lambda_filter, mu, filter_scope, ctx):
        from . import mesh_ops
        vert, nrm, col = mesh_ops.smooth(self.vertices, self.triangles, kind, number_of_iterations, lambda_filter, mu, filter_scope,
                                         self.vertex_normals if self.has_vertex_normals() else None,
                                         self.vertex_colors if self.has_vertex_colors() else None, ctx=ctx)
        out = TriangleMesh(vert, self.triangles.copy(), col, nrm)
        if self.triangle_normals is not None:
            out.triangle_normals = self.triangle_normals.copy()
        return out

    def filter_smooth_simple(self, number_of_iterations=1, filter_scope=0, ctx=None):
        """every vertex becomes the mean of itself and its neighbours, number_of_iterations times"""
        from . import mesh_ops
        return self._filtered(mesh_ops.SMOOTH_SIMPLE, number_of_iterations, 0.0, 0.0, filter_scope, ctx)

    def filter_smooth_laplacian(self, number_of_iterations=1, lambda_filter=0.5, filter_scope=0, ctx=None):
        """v += lambda (inverse-distance weighted mean of the neighbours - v), number_of_iterations times (mesh_reconstruction.py:22-37)"""
        from . import mesh_ops
        return self._filtered(mesh_ops.SMOOTH_LAPLACIAN, number_of_iterations, lambda_filter, 0.0, filter_scope, ctx)

    def filter_smooth_taubin(self, number_of_iterations=1, lambda_filter=0.5, mu=-0.53, filter_scope=0, ctx=None):
        """a Laplacian step with lambda, then one with mu, number_of_iterations times: smooths without the shrinkage"""
        from . import mesh_ops
        return self._filtered(mesh_ops.SMOOTH_TAUBIN, number_of_iterations, lambda_filter, mu, filter_scope, ctx)

    # ---- clean-ups: in place, survivors keep their order, colours and normals travel with their vertices
    def _compact(self, flags=0, vertex_keep=None, triangle_keep=None, ctx=None):
        from . import mesh_ops
        vert, tri, nrm, col = mesh_ops.compact(self.vertices, self.triangles, flags, vertex_keep, triangle_keep,
                                               self.vertex_normals if self.has_vertex_normals() else None,
                                               self.vertex_colors if self.has_vertex_colors() else None, ctx=ctx)
        if len(tri) != len(self.triangles):
            self.triangle_normals = None            # recompute them: which triangles went is not reported
        self.vertices, self.triangles = vert, tri
        # an attribute array that did not match the vertices (has_* false) was not carried: it becomes empty, None stays None
        self.vertex_normals = nrm if nrm is not None or self.vertex_normals is None else np.zeros((0, 3))
        self.vertex_colors = col if col is not None or self.vertex_colors is None else np.zeros((0, 3))
        self.adjacency_list = None
        return self

    def remove_degenerate_triangles(self, ctx=None):
        """drops triangles with two equal indices"""
        from . import mesh_ops
        return self._compact(mesh_ops.DROP_DEGENERATE, ctx=ctx)

    def remove_unreferenced_vertices(self, ctx=None):
        from . import mesh_ops
        return self._compact(mesh_ops.DROP_UNREFERENCED, ctx=ctx)

    def remove_vertices_by_mask(self, vertex_mask, ctx=None):
        """vertex_mask: truthy where a vertex is REMOVED (Open3D's sense); also drops every triangle that touches one"""
        keep = ~(np.asarray(vertex_mask).reshape(-1) != 0)
        return self._compact(0, vertex_keep=keep, ctx=ctx)

    def remove_triangles_by_mask(self, triangle_mask, ctx=None):
        """triangle_mask: truthy where a triangle is REMOVED"""
        keep = ~(np.asarray(triangle_mask).reshape(-1) != 0)
        return self._compact(0, triangle_keep=keep, ctx=ctx)

    def remove_non_finite_vertices(self, ctx=None):
        """the scrub of check84.py:315-322: remove_vertices_by_mask of the rows with a NaN or an infinity"""
        from . import mesh_ops
        return self._compact(mesh_ops.DROP_NON_FINITE, ctx=ctx)

    # ---- topology (mesh_ops.py, csrc/meshtopo.hip): the edge table, connected components and the welds
    def cluster_connected_triangles(self, ctx=None):
        """-> triangle_clusters int32 [m], cluster_n_triangles int64 [], cluster_area float64 []: triangles that share an edge are
        connected; the components are numbered in ascending order of their lowest triangle"""
        from . import mesh_ops
        return mesh_ops.components(self.vertices, self.triangles, ctx=ctx)

    def remove_small_components(self, min_triangles=0, min_area=0.0, keep_largest=False, ctx=None):
        """the tutorial idiom: cluster_connected_triangles, then the components with fewer than min_triangles triangles or less than
        min_area area go (keep_largest: all but the one with the most triangles), with the vertices they leave unreferenced"""
        from . import mesh_ops
        labels, count, area = mesh_ops.components(self.vertices, self.triangles, ctx=ctx)
        gone = mesh_ops.component_mask(labels, count, area, min_triangles, min_area, keep_largest)
        if gone.any():
            self.remove_triangles_by_mask(gone, ctx=ctx)
        return self.remove_unreferenced_vertices(ctx=ctx)

    def _dedup(self, flags, ctx):
        from . import mesh_ops
        vert, tri, nrm, col, _, origin = mesh_ops.dedup(self.vertices, self.triangles, flags,
                                                        self.vertex_normals if self.has_vertex_normals() else None,
                                                        self.vertex_colors if self.has_vertex_colors() else None, ctx=ctx)
        if self.triangle_normals is not None:
            self.triangle_normals = self.triangle_normals[origin] if len(self.triangle_normals) == len(self.triangles) else None
        self.vertices, self.triangles = vert, tri
        self.vertex_normals = nrm if nrm is not None or self.vertex_normals is None else np.zeros((0, 3))
        self.vertex_colors = col if col is not None or self.vertex_colors is None else np.zeros((0, 3))
        self.adjacency_list = None
        return self

    def remove_duplicated_vertices(self, ctx=None):
        """vertices with equal x, y and z (as doubles: -0.0 == +0.0, a NaN equals nothing) become the first of them, which keeps its
        own normal and colour; triangles are renumbered, none is dropped"""
        from . import mesh_ops
        return self._dedup(mesh_ops.DEDUP_VERTICES, ctx)

    def remove_duplicated_triangles(self, ctx=None):
        """triangles equal up to rotation become the first of them ((a,c,b) is another triangle than (a,b,c)); triangle_normals follow"""
        from . import mesh_ops
        return self._dedup(mesh_ops.DEDUP_TRIANGLES, ctx)

    def _edge_table(self, ctx):
        from . import mesh_ops
        return mesh_ops.edges(len(self.vertices), self.triangles, ctx=ctx)

    def get_non_manifold_edges(self, allow_boundary_edges=True, ctx=None):
        """-> int32 [k,2] (min, max) ascending: the edges with more than two sides on them; allow_boundary_edges=False adds the
        edges with one (every edge whose count is not 2).  Open3D's order is its hash map's."""
        edg, cnt, _ = self._edge_table(ctx)
        return edg[cnt > 2 if allow_boundary_edges else cnt != 2]

    def is_edge_manifold(self, allow_boundary_edges=True, ctx=None):
        _, _, stats = self._edge_table(ctx)
        return bool(stats[2] == 0 and (allow_boundary_edges or stats[1] == 0))

    def euler_poincare_characteristic(self, ctx=None):
        """V + F - E with every vertex counted, referenced or not, as Open3D does"""
        _, _, stats = self._edge_table(ctx)
        return int(len(self.vertices) + len(self.triangles) - stats[0])

    def __iadd__(self, other):
        """Open3D's operator+=: the other mesh's vertices and triangles behind this one's, its indices offset; colours, vertex
        normals and triangle normals stay only when both meshes have them (an empty mesh has everything)"""
        if not len(other.vertices):
            return self
        nv = len(self.vertices)

        def both(mine, theirs, have, n_mine):
            return np.concatenate([mine, theirs]) if theirs is not None and (n_mine == 0 or have) else None
        colors = both(self.vertex_colors if nv else np.zeros((0, 3)), other.vertex_colors if other.has_vertex_colors() else None, self.has_vertex_colors(), nv)
        normals = both(self.vertex_normals if nv else np.zeros((0, 3)), other.vertex_normals if other.has_vertex_normals() else None,
                       self.has_vertex_normals(), nv)
        nt = len(self.triangles)
        tnormals = both(self.triangle_normals if nt else np.zeros((0, 3)), other.triangle_normals if other.has_triangle_normals() else None,
                        self.has_triangle_normals(), nt)
        self.vertices = np.concatenate([self.vertices, other.vertices])
        self.triangles = np.ascontiguousarray(np.concatenate([self.triangles, other.triangles + np.int32(nv)]), dtype=np.int32)
        self.vertex_colors, self.vertex_normals, self.triangle_normals = colors, normals, tnormals
        self.adjacency_list = None
        return self

    def __add__(self, other):
        out = TriangleMesh(self.vertices.copy(), self.triangles.copy(), None if self.vertex_colors is None else self.vertex_colors.copy(),
                           None if self.vertex_normals is None else self.vertex_normals.copy())
        out.triangle_normals = None if self.triangle_normals is None else self.triangle_normals.copy()
        out += other
        return out

    def transform(self, T):
        from . import cloud_ops
        T = np.asarray(T, dtype=np.float64)
        if len(self.vertices):
            self.vertices = cloud_ops.transform_points(self.vertices, T)
        if self.has_vertex_normals():
            self.vertex_normals = cloud_ops.transform_points(self.vertex_normals, T, rotate_only=True)
        return self


def as_arrays(pcd):
    """(points, colors|None, normals|None) float64 arrays from a PointCloud-like object or an (N,3) array."""
    if isinstance(pcd, np.ndarray):
        return _arr(pcd), None, None
    p = _arr(pcd.points)
    c = _arr(getattr(pcd, "colors", None))
    n = _arr(getattr(pcd, "normals", None))
    return p, (c if len(c) == len(p) and len(p) else None), (n if len(n) == len(p) and len(p) else None)


def like(template, points, colors=None, normals=None):
    """Builds the result in the caller's own cloud type when it is constructible and assignable, else PointCloud."""
    if isinstance(template, (PointCloud, np.ndarray)) or template is None:
        return PointCloud(points, colors, normals)
    try:
        out = type(template)()
        vec = type(template.points)
        out.points = vec(points)
        if colors is not None:
            out.colors = vec(colors)
        if normals is not None:
            out.normals = vec(normals)
        return out
    except Exception:  # noqa: BLE001
        return PointCloud(points, colors, normals)
