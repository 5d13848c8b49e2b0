"""GPU tests of the pose-graph optimisation ("Pose-graph optimisation"): the linearisation, the solve and the
whole of global_optimization, each bit for bit against tests/posegraph_ref.py (np.array_equal, no tolerance), on the smallest
shapes where the kernels can go wrong: 6 N = 258 is just past 256 and a multiple of no tile, order 1026 is past 1024 and takes more
than one panel, block and tile at the sizes 32, 64 and 256; order 1100 puts the rows below a panel into two workgroups of 1024."""
import ctypes
import json
import os

import numpy as np
import pytest

from tests import posegraph_ref as ref
from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu

RING_CLOSURES = [(0, 6), (3, 9), (2, 7)]


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError(f"{what}: {len(bad)} of {got.size} entries differ, first at {bad[0]}: {got[tuple(bad[0])]!r} != {want[tuple(bad[0])]!r}")


def _params(r3d, option=None, criteria=None):
    pg = r3d.posegraph
    return pg.posegraph_params(pg.GlobalOptimizationConvergenceCriteria(**(criteria or {})), pg.GlobalOptimizationOption(**(option or {})))


def _device(r3d, g, option=None, criteria=None):
    return r3d.posegraph.optimize(g.poses, g.nodes, g.T, g.info, g.uncertain, g.confidence, _params(r3d, option, criteria), trace=True)


def _check_run(r3d, g, option=None, criteria=None, twice=False):
    """the device's global_optimization of g against the restatement's: poses, confidences, kept, counts, objectives, trace"""
    h = g.copy()
    want = ref.global_optimization(h, option, criteria)
    got = _device(r3d, g, option, criteria)
    st = got["stats"]
    assert (st["outer_iterations"], st["trials"], st["rejected_trials"], st["failed_factorizations"], st["edges_pruned"]) == \
        (want["outer"], want["trials"], want["rejected"], want["failed"], want["pruned"]), (st, {k: v for k, v in want.items() if k != "trace"})
    assert (st["stop_first"], st["stop_second"]) == want["stops"]
    _same(got["trace"], want["trace"], "trace")
    _same(got["poses"], h.poses, "poses")
    _same(got["confidence"], h.confidence, "confidence")
    _same(got["kept"], h.kept, "kept")
    assert (st["first_objective"], st["final_objective"]) == (want["first"], want["final"])
    if twice:
        again = _device(r3d, g, option, criteria)
        for key in ("poses", "confidence", "kept", "trace"):
            assert got[key].tobytes() == again[key].tobytes(), key
    return got, want, h


# ---- r3d_debug_posegraph_linearize -------------------------------------------------------------------------------------------------
def _check_linearize(r3d, g):
    want_e, want_l, want_H, want_b, q = ref.linearize(g)
    mu = ref.line_process_mu(g, ref.DEFAULT_OPTION)
    got = r3d.posegraph.debug_linearize(g.poses, g.nodes, g.T, g.info, g.uncertain, g.confidence)
    _same(got["e"], want_e, "e")
    _same(got["l"], want_l, "l")
    _same(got["b"], want_b, "b")
    _same(got["H"], want_H, "H")
    assert got["F"] == ref.objective(g, q, want_l, mu)
    return got


def test_linearize_one_edge(r3d):
    rng = np.random.default_rng(2)
    g = ref.Graph([ref.random_pose(rng), ref.random_pose(rng)], [(0, 1)], [ref.random_pose(rng)], [ref.random_info(rng)], [False])
    _check_linearize(r3d, g)


def test_linearize_repeated_pairs_both_kinds_and_an_isolated_node(r3d):
    """N = 5: two edges between the same pair (one certain, one uncertain), an edge with s > t and its reverse, node 3 without an edge"""
    rng = np.random.default_rng(3)
    nodes = [(0, 1), (0, 1), (4, 2), (2, 4), (1, 0), (4, 0)]
    unc = [False, True, True, False, True, False]
    conf = [1.0, 0.37, 0.81, 1.0, 0.5, 1.0]
    g = ref.Graph([ref.random_pose(rng) for _ in range(5)], nodes, [ref.random_pose(rng) for _ in nodes], [ref.random_info(rng) for _ in nodes], unc, conf)
    got = _check_linearize(r3d, g)
    assert not got["H"][18:24].any() and not got["H"][:, 18:24].any() and not got["b"][18:24].any()


def test_linearize_258_unknowns_uneven_degrees(r3d):
    g = ref.random_graph(43, 200, seed=4)
    deg = np.bincount(g.nodes.reshape(-1), minlength=43)
    assert deg.max() >= 10 * max(1, deg[deg > 0].min())
    _check_linearize(r3d, g)


# ---- r3d_debug_posegraph_solve -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def systems():
    return {n: ref.spd(n, seed=n) for n in (6, 30, 258, 1026)}


@pytest.mark.parametrize("n", [6, 30, 258, 1026])
@pytest.mark.parametrize("lam", [0.0, 1.0])
def test_solve(r3d, systems, n, lam):
    A, b = systems[n]
    want_L, want_d, fail = ref.solve(A, b, lam)
    assert fail == -1
    L, d, got_fail = r3d.posegraph.debug_solve(A, b, lam)
    assert got_fail == -1
    _same(L, want_L, "L")
    _same(d, want_d, "delta")
    assert not np.triu(L, 1).any()                      # the documented strict upper triangle: zero


def test_solve_rows_below_a_panel_in_two_workgroups(r3d):
    """order 1100: the first two panels have more than 1024 rows below them, which k_pg_panel spreads over two workgroups (one
    factors and publishes the diagonal tile, both read it)"""
    A, b = ref.spd(1100, seed=11)
    want_L, want_d, _ = ref.solve(A, b, 0.5)
    L, d, fail = r3d.posegraph.debug_solve(A, b, 0.5)
    assert fail == -1
    _same(L, want_L, "L")
    _same(d, want_d, "delta")


def test_solve_failed_pivot(r3d, systems):
    """the 200th pivot goes negative: the flag names it and nothing that is not finite comes back"""
    A, b = systems[258]
    A = A.copy()
    L, _ = ref.cholesky_columns(A)
    A[199, 199] -= L[199, 199] * L[199, 199] + 1.0
    want_L, want_d, fail = ref.solve(A, b, 0.0)
    assert fail == 199
    L, d, got_fail = r3d.posegraph.debug_solve(A, b, 0.0)
    assert got_fail == 199
    assert np.isfinite(L).all() and np.isfinite(d).all() and not L.any() and not d.any()
    # the same context solves the untouched system afterwards
    A, b = systems[258]
    _same(r3d.posegraph.debug_solve(A, b, 0.0)[1], ref.solve(A, b, 0.0)[1], "delta after a failed solve")


# ---- r3d_posegraph_optimize --------------------------------------------------------------------------------------------------------
def test_ring_converges(r3d):
    g, truth = ref.ring(12, seed=1)
    got, want, h = _check_run(r3d, g, dict(reference_node=0), twice=True)
    assert np.abs(got["poses"] - truth).max() < 1e-4 and got["stats"]["edges_pruned"] == 0


def test_ring_prunes_the_wrong_closure(r3d):
    g, truth = ref.ring(12, closures=RING_CLOSURES, wrong=(3, 9), seed=1)
    got, want, h = _check_run(r3d, g, dict(reference_node=0), twice=True)
    assert got["kept"].tolist() == [True] * 12 + [True, False, True] and got["stats"]["edges_pruned"] == 1
    assert got["confidence"][12] > 0.25 and got["confidence"][14] > 0.25 and got["confidence"][13] < 0.25


def _chain(r3d, n=6, seed=5):
    rng = np.random.default_rng(seed)
    edges = [dict(source=k + 1, target=k, T=ref.random_pose(rng, 0.1, 0.2), info=ref.random_info(rng), uncertain=False) for k in range(n - 1)]
    return edges, np.stack(r3d.pipeline.poses_from_edges(edges))


def test_chain_stops_before_the_first_trial(r3d):
    edges, poses = _chain(r3d)
    g = ref.Graph(poses, [(e["source"], e["target"]) for e in edges], [e["T"] for e in edges], [e["info"] for e in edges], [False] * len(edges))
    got, want, _ = _check_run(r3d, g, dict(reference_node=0))
    assert got["stats"]["trials"] == 0 and got["stats"]["stop_first"] == ref.STOP_RIGHT_TERM
    assert got["poses"].tobytes() == poses.tobytes()
    assert [p.tobytes() for p in r3d.pipeline.optimize_poses(edges)] == [p.tobytes() for p in poses]


def test_single_node_without_edges(r3d):
    pose = ref.random_pose(np.random.default_rng(6))
    got = r3d.posegraph.optimize([pose], np.zeros((0, 2), np.int32), np.zeros((0, 16)), np.zeros((0, 36)), [], None, trace=True)
    assert got["poses"].tobytes() == pose.tobytes() and got["stats"]["trials"] == 0 and len(got["trace"]) == 0
    assert got["stats"]["stop_first"] == got["stats"]["stop_second"] == ref.STOP_NO_EDGES


@pytest.mark.parametrize("node", [0, 11, -1])
def test_reference_node(r3d, node):
    g, _ = ref.ring(12, closures=RING_CLOSURES[:1], seed=7)
    before = g.poses.copy()
    got, _, _ = _check_run(r3d, g, dict(reference_node=node), dict(max_iteration=4))
    if node >= 0:
        assert np.array_equal(got["poses"][node], before[node])       # the same values; I X may turn a -0 of X into +0
    assert got["stats"]["trials"] >= 3


def test_device_form_equals_host_form(r3d):
    g, _ = ref.ring(12, closures=RING_CLOSURES, wrong=(3, 9), seed=1)
    prm = _params(r3d, dict(reference_node=0))
    host = _device(r3d, g, dict(reference_node=0))
    ctx = r3d.default_context()
    arrays = r3d.posegraph.graph_arrays(g.poses, g.nodes, g.T, g.info, g.uncertain, g.confidence)
    dev = [ctx.to_device(a) for a in arrays]
    E = len(g.nodes)
    d_kept, d_trace = ctx.alloc(E), ctx.alloc(host["stats"]["trials"] * 32)
    try:
        prm.trace_capacity = host["stats"]["trials"]
        st = r3d.posegraph.optimize_device(dev[0], 12, E, dev[1], dev[2], dev[3], dev[4], dev[5], d_kept, prm, d_trace)
        poses, conf, kept, trace = np.empty((12, 4, 4)), np.empty(E), np.empty(E, np.uint8), np.empty((host["stats"]["trials"], 4))
        for arr, ptr in ((poses, dev[0]), (conf, dev[5]), (kept, d_kept), (trace, d_trace)):
            ctx.d2h(arr, ptr)
    finally:
        for ptr in dev + [d_kept, d_trace]:
            ctx.free(ptr)
    _same(poses, host["poses"], "poses")
    _same(conf, host["confidence"], "confidence")
    _same(kept.astype(bool), host["kept"], "kept")
    _same(trace, host["trace"], "trace")
    assert {k: v for k, v in st.items() if not k.endswith("_ms")} == {k: v for k, v in host["stats"].items() if not k.endswith("_ms")}


def test_refusals_leave_the_context_usable(r3d):
    """every refusal of include/r3d.h, asked of the library itself (the Python layer would turn most of them down first)"""
    ctx = r3d.default_context()
    lib = r3d._lib.load()
    g, _ = ref.ring(4, seed=8)

    def call(g, N=None, E=None, **prm):
        p = _params(r3d)
        for k, v in prm.items():
            setattr(p, k, v)
        poses, nodes = g.poses.reshape(-1, 16).copy(), np.ascontiguousarray(g.nodes, dtype=np.int32)
        T, info = np.ascontiguousarray(g.T.reshape(-1, 16)), np.ascontiguousarray(g.info.reshape(-1, 36))
        unc, conf, kept = g.uncertain.astype(np.uint8), g.confidence.copy(), np.zeros(len(g.nodes), np.uint8)
        rc = lib.r3d_posegraph_optimize(ctx._h, ctypes.byref(p), len(poses) if N is None else N, _p(poses), len(nodes) if E is None else E, _p(nodes),
                                        _p(T), _p(info), _p(unc), _p(conf), _p(kept), None, None)
        return rc, (lib.r3d_last_error(ctx._h) or b"").decode(), poses.tobytes() == g.poses.reshape(-1, 16).tobytes()

    def broken(field, index, value):
        h = g.copy()
        getattr(h, field)[index] = value
        return h
    cases = [call(g, N=0), call(g, N=1025), call(g, E=(1 << 20) + 1), call(g, E=-1), call(broken("nodes", (1, 0), 4)), call(broken("nodes", (1, 1), -1)),
             call(broken("nodes", (2, 0), int(g.nodes[2, 1]))), call(broken("poses", (1, 0, 3), np.nan)), call(broken("T", (0, 2, 2), np.inf)),
             call(broken("info", (3, 5, 5), np.nan)), call(g, reference_node=4), call(g, reference_node=-2), call(g, max_iteration=-1),
             call(g, max_iteration_lm=-1)]
    for k, (rc, msg, untouched) in enumerate(cases):
        assert rc == -1 and msg and untouched, (k, rc, msg, untouched)
    rc, _, _ = call(g)
    assert rc == 0
    _check_run(r3d, g, dict(reference_node=0), dict(max_iteration=2))


def test_1026_unknowns_three_iterations(r3d):
    g = ref.random_graph(171, 500, seed=9, hub=False)
    got, want, _ = _check_run(r3d, g, dict(reference_node=0), dict(max_iteration=3))
    assert got["stats"]["outer_iterations"] == 6 and got["stats"]["trials"] >= 6


# ---- pipeline ----------------------------------------------------------------------------------------------------------------------
def test_recorded_frames_through_the_pose_graph(r3d):
    """frames 8-11 of the recorded scan (its one colour image with each depth map): odometry edges plus the closures between every
    pair of frames, optimised; the result is the restatement's on the same edges, and tsdf_fuse takes it"""
    from PIL import Image
    color = np.asarray(Image.open(os.path.join(GOLDEN, "output84/color_00008.png")))
    frames = [(color, np.asarray(Image.open(os.path.join(GOLDEN, f"output84/depth_{i:05d}.png"))).astype(np.uint16)) for i in range(8, 12)]
    cam = r3d.cloud_ops.depth_camera(json.load(open(os.path.join(GOLDEN, "camera_intrinsic.json"))), depth_scale=1000.0, depth_trunc=3.0)
    edges = r3d.pipeline.odometry_edges(frames, cam)
    loops = r3d.pipeline.loop_closure_edges(frames, cam, every=1)
    assert [(e["source"], e["target"]) for e in edges] == [(1, 0), (2, 1), (3, 2)]
    assert all(e["uncertain"] and e["source"] - e["target"] > 1 for e in loops) and {(e["source"], e["target"]) for e in loops} <= {(2, 0), (3, 0), (3, 1)}
    poses = r3d.pipeline.optimize_poses(edges, loops)
    both = edges + loops
    g = ref.Graph(r3d.pipeline.poses_from_edges(edges), [(e["source"], e["target"]) for e in both], [e["T"] for e in both], [e["info"] for e in both],
                  [e["uncertain"] for e in both])
    ref.global_optimization(g, dict(reference_node=0))
    _same(np.stack(poses), g.poses, "poses")
    graph = r3d.pipeline.pose_graph_from_edges(both, r3d.pipeline.poses_from_edges(edges))
    assert len(graph.nodes) == 4 and len(graph.edges) == len(both)
    cloud = r3d.pipeline.tsdf_fuse(frames, cam, poses, 0.02, 0.08)
    assert len(cloud) > 1000 and np.isfinite(np.asarray(cloud.points)).all()
