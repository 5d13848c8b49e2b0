"""o3d.pipelines.registration.global_optimization on the device ("Pose-graph optimisation"; C ABI:
r3d_posegraph_*): Levenberg-Marquardt over a pose graph with a line process on the uncertain (loop-closure) edges, float64, every
sum in a fixed order.  Parity with Open3D is UNPINNED; tests/posegraph_ref.py restates the contract and the device result equals it
bit for bit."""
import ctypes

import numpy as np

from . import _lib
from ._lib import PoseGraphParams, PoseGraphStats

_vp = ctypes.c_void_p
MAX_NODES, MAX_EDGES = 1024, 1 << 20
STOP_NAMES = {0: "none", 1: "right term", 2: "relative increment", 3: "relative residual increment", 4: "residual", 5: "iterations", 6: "no edges"}


class PoseGraphNode:
    """a camera-to-world pose, 4x4"""

    def __init__(self, pose=None):
        self.pose = np.eye(4) if pose is None else np.array(pose, dtype=np.float64).reshape(4, 4)


class PoseGraphEdge:
    """transformation maps source camera coordinates to target camera coordinates; information is 6x6; an uncertain edge (a loop
    closure) is weighted by its confidence, which the optimisation rewrites"""

    def __init__(self, source_node_id=-1, target_node_id=-1, transformation=None, information=None, uncertain=False, confidence=1.0):
        self.source_node_id, self.target_node_id = int(source_node_id), int(target_node_id)
        self.transformation = np.eye(4) if transformation is None else np.array(transformation, dtype=np.float64).reshape(4, 4)
        self.information = np.eye(6) if information is None else np.array(information, dtype=np.float64).reshape(6, 6)
        self.uncertain, self.confidence = bool(uncertain), float(confidence)


class PoseGraph:
    def __init__(self, nodes=None, edges=None):
        self.nodes, self.edges = list(nodes or []), list(edges or [])


class GlobalOptimizationLevenbergMarquardt:
    """the one method there is (Open3D's GlobalOptimizationGaussNewton is not built)"""


class GlobalOptimizationConvergenceCriteria:
    def __init__(self, max_iteration=100, min_relative_increment=1e-6, min_relative_residual_increment=1e-6, min_right_term=1e-6,
                 min_residual=1e-6, max_iteration_lm=20, upper_scale_factor=2.0 / 3.0, lower_scale_factor=1.0 / 3.0):
        self.max_iteration, self.max_iteration_lm = int(max_iteration), int(max_iteration_lm)
        self.min_relative_increment, self.min_relative_residual_increment = float(min_relative_increment), float(min_relative_residual_increment)
        self.min_right_term, self.min_residual = float(min_right_term), float(min_residual)
        # kept for Open3D's signature; the lambda update of the contract is max(1/3, 1 - (2 rho - 1)^3) and reads neither
        self.upper_scale_factor, self.lower_scale_factor = float(upper_scale_factor), float(lower_scale_factor)


class GlobalOptimizationOption:
    def __init__(self, max_correspondence_distance=0.03, edge_prune_threshold=0.25, preference_loop_closure=1.0, reference_node=-1):
        self.max_correspondence_distance, self.edge_prune_threshold = float(max_correspondence_distance), float(edge_prune_threshold)
        self.preference_loop_closure, self.reference_node = float(preference_loop_closure), int(reference_node)


def posegraph_params(criteria=None, option=None, trace_capacity=0):
    c, o = criteria or GlobalOptimizationConvergenceCriteria(), option or GlobalOptimizationOption()
    return PoseGraphParams(o.max_correspondence_distance, o.edge_prune_threshold, o.preference_loop_closure, c.min_relative_increment,
                           c.min_relative_residual_increment, c.min_right_term, c.min_residual, o.reference_node, c.max_iteration, c.max_iteration_lm,
                           int(trace_capacity))


_ptr = _lib.ptr


def _refuse(msg):
    raise _lib.R3DError(-1, "posegraph: " + msg)


def graph_arrays(poses, nodes, T, info, uncertain, confidence=None):
    """The arrays of the C entry points from anything array-like, with the refusals that need no device (R3D_E_BADARG)
    -> poses [N,16], nodes int32 [E,2], T [E,16], info [E,36], uncertain uint8 [E], confidence [E]"""
    poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 16).copy()
    nodes = np.ascontiguousarray(nodes, dtype=np.int32).reshape(-1, 2)
    E, N = len(nodes), len(poses)
    T = np.ascontiguousarray(T, dtype=np.float64).reshape(-1, 16)
    info = np.ascontiguousarray(info, dtype=np.float64).reshape(-1, 36)
    uncertain = np.ascontiguousarray(np.asarray(uncertain, dtype=bool).reshape(-1), dtype=np.uint8)
    confidence = np.ones(E) if confidence is None else np.ascontiguousarray(confidence, dtype=np.float64).reshape(-1).copy()
    if not (len(T) == len(info) == len(uncertain) == len(confidence) == E):
        _refuse(f"{E} edges but {len(T)} transformations, {len(info)} information matrices, {len(uncertain)} flags, {len(confidence)} confidences")
    if N < 1 or N > MAX_NODES:
        _refuse(f"{N} nodes (1..{MAX_NODES} are supported)")
    if E > MAX_EDGES:
        _refuse(f"{E} edges (at most 2^20 are supported)")
    if E and (nodes.min() < 0 or nodes.max() >= N):
        _refuse("an edge names a node outside 0..n_nodes-1")
    if E and (nodes[:, 0] == nodes[:, 1]).any():
        _refuse("an edge joins a node to itself")
    if not (np.isfinite(poses).all() and np.isfinite(T).all() and np.isfinite(info).all() and np.isfinite(confidence).all()):
        _refuse("a pose, transformation, information matrix or confidence that is not finite")
    return poses, nodes, T, info, uncertain, confidence


def _check_params(prm, N):
    if not -1 <= prm.reference_node < N:
        _refuse(f"reference_node {prm.reference_node} is outside -1..{N - 1}")
    if prm.max_iteration < 0 or prm.max_iteration_lm < 0:
        _refuse("a negative iteration count")


def _stats_dict(st):
    return {n: getattr(st, n) for n, _ in PoseGraphStats._fields_ if n != "reserved"}


def optimize(poses, nodes, T, info, uncertain, confidence=None, params=None, trace=False, ctx=None):
    """r3d_posegraph_optimize on arrays -> dict(poses [N,4,4], confidence [E], kept bool [E], stats dict, trace [trials,4] or None)"""
    prm = params or posegraph_params()
    poses, nodes, T, info, uncertain, confidence = graph_arrays(poses, nodes, T, info, uncertain, confidence)
    _check_params(prm, len(poses))
    ctx = ctx or _lib.default_context()
    E = len(nodes)
    if trace:
        prm = PoseGraphParams.from_buffer_copy(prm)
        prm.trace_capacity = max(1, min(2 * prm.max_iteration * max(1, prm.max_iteration_lm), 1 << 20))
    rows = np.zeros((prm.trace_capacity, 4)) if trace else None
    kept, st = np.ones(E, np.uint8), PoseGraphStats()
    ctx.call("r3d_posegraph_optimize", ctypes.byref(prm), len(poses), _ptr(poses), E, _ptr(nodes), _ptr(T), _ptr(info), _ptr(uncertain),
             _ptr(confidence), _ptr(kept), ctypes.byref(st), _ptr(rows))
    return dict(poses=poses.reshape(-1, 4, 4), confidence=confidence, kept=kept.astype(bool), stats=_stats_dict(st),
                trace=rows[:min(st.trials, len(rows))].copy() if trace else None)


def optimize_device(d_poses, n_nodes, n_edges, d_nodes, d_T, d_info, d_uncertain, d_confidence, d_kept, params=None, d_trace=None, ctx=None):
    """r3d_posegraph_optimize_dev: device pointers (int); poses and confidences are rewritten in place -> stats dict"""
    ctx = ctx or _lib.default_context()
    prm = params or posegraph_params()
    st = PoseGraphStats()
    ctx.call("r3d_posegraph_optimize_dev", ctypes.byref(prm), int(n_nodes), _vp(d_poses), int(n_edges), _vp(d_nodes), _vp(d_T), _vp(d_info),
             _vp(d_uncertain), _vp(d_confidence), _vp(d_kept), ctypes.byref(st), _vp(d_trace))
    return _stats_dict(st)


def debug_linearize(poses, nodes, T, info, uncertain, confidence=None, params=None, ctx=None):
    """r3d_debug_posegraph_linearize -> dict(e [E,6], l [E], H [6N,6N], b [6N], F)"""
    prm = params or posegraph_params()
    poses, nodes, T, info, uncertain, confidence = graph_arrays(poses, nodes, T, info, uncertain, confidence)
    ctx = ctx or _lib.default_context()
    E, n = len(nodes), 6 * len(poses)
    out = dict(e=np.full((E, 6), np.nan), l=np.full(E, np.nan), H=np.full((n, n), np.nan), b=np.full(n, np.nan))
    F = ctypes.c_double()
    ctx.call("r3d_debug_posegraph_linearize", ctypes.byref(prm), len(poses), _ptr(poses), E, _ptr(nodes), _ptr(T), _ptr(info), _ptr(uncertain),
             _ptr(confidence), _ptr(out["e"]), _ptr(out["l"]), _ptr(out["H"]), _ptr(out["b"]), ctypes.byref(F))
    out["F"] = F.value
    return out


def debug_solve(A, b, lam, ctx=None):
    """r3d_debug_posegraph_solve: (A + lam I) delta = -b -> L [n,n] (strict upper triangle zero), delta [n], failed pivot or -1"""
    ctx = ctx or _lib.default_context()
    A = np.ascontiguousarray(A, dtype=np.float64)
    n = len(A)
    b = np.ascontiguousarray(b, dtype=np.float64).reshape(n)
    L, delta, fail = np.full((n, n), np.nan), np.full(n, np.nan), ctypes.c_int32(-1)
    ctx.call("r3d_debug_posegraph_solve", n, _ptr(A), _ptr(b), float(lam), _ptr(L), _ptr(delta), ctypes.byref(fail))
    return L, delta, fail.value


def global_optimization(pose_graph, method=None, criteria=None, option=None, ctx=None):
    """o3d.pipelines.registration.global_optimization(pose_graph, method, criteria, option): in place.  The node poses and the edge
    confidences are rewritten and the pruned edges leave pose_graph.edges, as in Open3D.  -> the stats dict (Open3D returns None)"""
    if method is not None and not isinstance(method, GlobalOptimizationLevenbergMarquardt):
        raise _lib.R3DError(-4, "global_optimization: only GlobalOptimizationLevenbergMarquardt is built")
    if not pose_graph.nodes:
        _refuse("a pose graph without nodes")
    ed = pose_graph.edges
    res = optimize([n.pose for n in pose_graph.nodes], [(e.source_node_id, e.target_node_id) for e in ed] or np.zeros((0, 2), np.int32),
                   [e.transformation for e in ed] or np.zeros((0, 16)), [e.information for e in ed] or np.zeros((0, 36)),
                   [e.uncertain for e in ed], [e.confidence for e in ed], posegraph_params(criteria, option), ctx=ctx)
    for node, pose in zip(pose_graph.nodes, res["poses"]):
        node.pose = pose.copy()
    for e, c in zip(ed, res["confidence"]):
        e.confidence = float(c)
    pose_graph.edges = [e for e, k in zip(ed, res["kept"]) if k]
    return res["stats"]
