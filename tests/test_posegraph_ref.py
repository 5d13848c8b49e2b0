"""CPU tests of the pose-graph restatement (tests/posegraph_ref.py): its two writings agree bit for bit, its Jacobian is the
derivative of its residual, its Cholesky solves within the derived backward error, and its optimisation does what the contract
promises on a ring of poses; then the parts of the package that need no device (JSON form, refusals, graph helpers)."""
import numpy as np
import pytest

from tests import posegraph_ref as ref

RING_CLOSURES = [(0, 6), (3, 9), (2, 7)]


def _small_graphs():
    rng = np.random.default_rng(2)
    one = ref.Graph([ref.random_pose(rng), ref.random_pose(rng)], [(0, 1)], [ref.random_pose(rng)], [ref.random_info(rng)], [False])
    rng = np.random.default_rng(3)
    nodes = [(0, 1), (0, 1), (4, 2), (2, 4), (1, 0), (4, 0)]
    five = ref.Graph([ref.random_pose(rng) for _ in range(5)], nodes, [ref.random_pose(rng) for _ in nodes], [ref.random_info(rng) for _ in nodes],
                     [False, True, True, False, True, False], [1.0, 0.37, 0.81, 1.0, 0.5, 1.0])
    return [one, five, ref.random_graph(43, 200, seed=4)]


# ---- the two writings ------------------------------------------------------------------------------------------------------------------
def test_sincos_two_writings_and_accuracy():
    """The contract's own sine and cosine.  Measured against numpy's on 400 000 uniform arguments: the absolute error is at most
    1 x 2^-53 for |x| < 4 and 2 x 2^-53 for |x| < 1e5 (the result is at most 1 in magnitude, so 2^-53 is half an ulp of 1); asserted
    at 2 x 2^-53 and 4 x 2^-53, twice the measurement, since numpy's own functions are within an ulp and not exact."""
    rng = np.random.default_rng(0)
    for span, units in ((4.0, 2.0), (1e5, 4.0)):
        x = rng.uniform(-span, span, 400000)
        s, c = ref.sincos(x)
        err = max(np.abs(s - np.sin(x)).max(), np.abs(c - np.cos(x)).max()) * 2.0 ** 53
        print(f"|x| < {span:g}: {err:.2f} x 2^-53")
        assert err <= units
        for v, a, b in zip(x[::4000], s[::4000], c[::4000]):
            assert ref.sincos_loops(v) == (a, b)
    assert ref.sincos(np.array([0.0]))[0][0] == 0.0 and ref.sincos(np.array([0.0]))[1][0] == 1.0
    assert np.isnan(ref.sincos(np.array([2.0 ** 30, np.inf, np.nan]))[0]).all() and np.isnan(ref.sincos_loops(2.0 ** 30)[0])
    assert np.array_equal(ref.exp6(np.zeros(6)), np.eye(4))


def test_algebra_two_writings():
    rng = np.random.default_rng(1)
    for _ in range(20):
        A, B, d = rng.normal(size=(4, 4)), rng.normal(size=(4, 4)), rng.normal(size=6)
        assert np.array_equal(ref.mul4(A, B), np.array(ref.mul4_loops(A.tolist(), B.tolist())))
        assert np.array_equal(ref.inv_rigid(A), np.array(ref.inv_rigid_loops(A.tolist())))
        assert np.array_equal(ref.vec6(A), np.array(ref.vec6_loops(A.tolist())))
        assert np.array_equal(ref.exp6(d), np.array(ref.exp6_loops(d.tolist())))
    X = ref.random_pose(rng)
    assert np.abs(ref.mul4(X, ref.inv_rigid(X)) - np.eye(4)).max() < 1e-15


@pytest.mark.parametrize("k", [0, 1, 2])
def test_linearize_two_writings(k):
    g = _small_graphs()[k]
    for a, b, name in zip(ref.linearize(g), ref.linearize_loops(g), ("e", "l", "H", "b", "q")):
        assert np.array_equal(a, b), name
    H = ref.linearize(g)[2]
    assert np.array_equal(H, H.T)


@pytest.fixture(scope="module")
def systems():
    return {n: ref.spd(n, seed=n) for n in (6, 30, 258, 1026)}


@pytest.mark.parametrize("n", [6, 30, 258, 1026])
def test_cholesky_writings_agree_whatever_the_tile(systems, n):
    A, b = systems[n]
    L, fail = ref.cholesky_columns(A)
    assert fail == -1 and not np.triu(L, 1).any()
    for tile in (32, 64, 256):
        Lt, ft = ref.cholesky_tiled(A, tile)
        assert ft == -1 and np.array_equal(L, Lt), tile
    if n <= 30:
        Ls, fs = ref.cholesky_loops(A)
        assert fs == -1 and np.array_equal(L, Ls)
    if n <= 258:
        assert np.array_equal(ref.substitute(L, -b), ref.substitute_loops(L, -b))


def test_cholesky_failed_pivot_in_every_writing(systems):
    A = systems[258][0].copy()
    L, _ = ref.cholesky_columns(A)
    A[199, 199] -= L[199, 199] * L[199, 199] + 1.0
    for fn in (ref.cholesky_columns, ref.cholesky_tiled, lambda M: ref.cholesky_tiled(M, 32)):
        Lf, fail = fn(A)
        assert fail == 199 and np.isfinite(Lf).all() and not Lf[:, 199:].any() and np.array_equal(Lf[:, :199], L[:, :199])
    small = np.array([[4.0, 2.0, 0.0], [2.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
    assert ref.cholesky_loops(small)[1] == ref.cholesky_columns(small)[1] == ref.cholesky_tiled(small)[1] == 1
    Lz, d, fail = ref.solve(A, systems[258][1], 0.0)
    assert fail == 199 and not d.any()


@pytest.mark.parametrize("n", [6, 30, 258, 1026])
@pytest.mark.parametrize("lam", [0.0, 1.0])
def test_solve_backward_error(systems, n, lam):
    """normwise backward error ||A d + b||inf / (||A||inf ||d||inf + ||b||inf) <= 4 n 2^-53: gamma_{3n+1} of Cholesky and two triangular
    solves (Higham, Accuracy and Stability of Numerical Algorithms, Theorem 10.4).  The residual is taken in longdouble."""
    A, b = systems[n]
    _, d, fail = ref.solve(A, b, lam)
    assert fail == -1
    Al = A.astype(np.longdouble) + np.longdouble(lam) * np.eye(n, dtype=np.longdouble)
    r = (Al * d.astype(np.longdouble)[None, :]).sum(1) + b.astype(np.longdouble)
    eta = float(np.abs(r).max() / (np.abs(Al).sum(1).max() * np.abs(d).max() + np.abs(b).max()))
    print(f"n = {n}, lambda = {lam}: backward error {eta:.3e}, bound {4 * n * 2.0 ** -53:.3e}")
    assert eta <= 4 * n * 2.0 ** -53
    x = np.linalg.solve(A + lam * np.eye(n), -b)
    assert np.abs(d - x).max() <= 1e-10 * np.abs(x).max()     # the two solutions of a system with a condition number below 100


def test_optimisation_two_writings():
    for g, option in ((ref.ring(12, seed=1)[0], dict(reference_node=0)),
                      (ref.ring(12, closures=RING_CLOSURES, wrong=(3, 9), seed=1)[0], dict(reference_node=0))):
        a, b = g.copy(), g.copy()
        ra = ref.global_optimization(a, option, dict(max_iteration=6), how="tiled", tile=32)
        rb = ref.global_optimization(b, option, dict(max_iteration=6), how="loops")
        assert np.array_equal(a.poses, b.poses) and np.array_equal(a.confidence, b.confidence) and np.array_equal(ra["trace"], rb["trace"])
        assert {k: v for k, v in ra.items() if k != "trace"} == {k: v for k, v in rb.items() if k != "trace"}


# ---- the Jacobian --------------------------------------------------------------------------------------------------------------------
def test_jacobian_against_central_differences():
    """J_s[:, k] against (e(+h) - e(-h)) / 2h with X_s <- exp6(h u_k) X_s, whose first-order term is G_k X_s.

    An entry of P exp6(h u_k) X_s is a combination of sin h, cos h and h with coefficients bounded by S = ||P||inf ||X_s||1 (P = inv(T)
    inv(X_t)), so its third derivative is at most S and the central difference is off by at most h^2 S / 6.  Each evaluation of e
    carries about 16 roundings of size 2^-53 S, which the division by 2h turns into 16 x 2^-53 S / h.  The sum is smallest near
    h = (48 x 2^-53)^(1/3) = 1.7e-5; h = 1e-5 is used and the bound is h^2 S / 6 + 16 x 2^-53 S / h per edge (S between 2 and 20 here:
    3e-11 .. 4e-10).  Measured on the 206 edges below: max |J - difference| = 2.81e-11, and at h = 1e-3, 1e-4 the error falls by 100 per
    decade (1.76e-7, 1.76e-9), which is the second-order remainder; J_t = -J_s holds exactly by construction."""
    worst = {}
    for g in _small_graphs()[1:]:
        e, J, _, _, _, _ = ref.edge_terms(g)
        s, t = g.nodes[:, 0], g.nodes[:, 1]
        P = ref.mul4(ref.inv_rigid(g.T), ref.inv_rigid(g.poses[t]))
        S = np.abs(P).sum(2).max(1) * np.abs(g.poses[s]).sum(1).max(1)
        for h in (1e-3, 1e-4, 1e-5):
            for k in range(6):
                u = np.zeros(6)
                u[k] = h
                up, dn = ref.exp6(u), ref.exp6(-u)
                ep = ref.vec6(ref.mul4(P, ref.mul4(up[None], g.poses[s])))
                em = ref.vec6(ref.mul4(P, ref.mul4(dn[None], g.poses[s])))
                err = np.abs((ep - em) / (2 * h) - J[:, :, k]).max(1)
                worst[h] = max(worst.get(h, 0.0), float(err.max()))
                if h == 1e-5:
                    assert (err <= h * h * S / 6 + 16 * 2.0 ** -53 * S / h).all(), (k, err.max())
                # the target's side: X_t <- exp6(h u_k) X_t gives -J_s to first order
                if h == 1e-5:
                    Pp = ref.mul4(ref.inv_rigid(g.T), ref.inv_rigid(ref.mul4(up[None], g.poses[t])))
                    Pm = ref.mul4(ref.inv_rigid(g.T), ref.inv_rigid(ref.mul4(dn[None], g.poses[t])))
                    et = (ref.vec6(ref.mul4(Pp, g.poses[s])) - ref.vec6(ref.mul4(Pm, g.poses[s]))) / (2 * h)
                    assert (np.abs(et + J[:, :, k]).max(1) <= h * h * S / 6 + 32 * 2.0 ** -53 * S / h).all()
    print({h: f"{v:.2e}" for h, v in worst.items()})
    assert worst[1e-4] < worst[1e-3] / 50 and worst[1e-5] < worst[1e-4] / 20


# ---- the optimisation ------------------------------------------------------------------------------------------------------------------
def test_ring_converges_to_the_truth():
    """12 poses on a ring, T from the truth, node poses perturbed by 0.02 (node 0, the reference node, is at its true pose, which
    fixes the gauge).  The optimisation stops at F < min_residual after 74 accepted trials; the largest entry of |pose - truth|
    falls from 6.58e-2 to 1.6425e-5 (measured with this restatement; min_residual = 1e-6 is what stops it there), and that figure
    is the bound."""
    g, truth = ref.ring(12, seed=1)
    before = np.abs(g.poses - truth).max()
    res = ref.global_optimization(g, dict(reference_node=0))
    err = np.abs(g.poses - truth).max()
    print(f"ring: {before:.3e} -> {err:.4e}, {res['trials']} trials, stops {res['stops']}")
    assert res["stops"][0] == ref.STOP_RESIDUAL and res["rejected"] == 0 and res["pruned"] == 0
    assert err <= 1.6425e-5 and np.array_equal(g.poses[0], truth[0])


def test_ring_prunes_exactly_the_wrong_closure():
    """three closures from the truth, the second one 0.5 m off: the line process takes its confidence to 2e-5, the other two stay
    above 0.99, the pruning drops exactly that edge and the second optimisation ends as close to the truth as the plain ring"""
    g, truth = ref.ring(12, closures=RING_CLOSURES, wrong=(3, 9), seed=1)
    res = ref.global_optimization(g, dict(reference_node=0))
    print(g.confidence[-3:], res["pruned"], np.abs(g.poses - truth).max())
    assert g.kept.tolist() == [True] * 12 + [True, False, True] and res["pruned"] == 1
    assert g.confidence[12] > 0.25 and g.confidence[14] > 0.25 and g.confidence[13] < 0.25
    assert np.abs(g.poses - truth).max() <= 2.1e-5
    assert (g.confidence[:12] == 1.0).all()                 # a certain edge's confidence is not touched


def test_chain_from_poses_from_edges_is_already_optimal(r3d):
    rng = np.random.default_rng(5)
    edges = [dict(source=k + 1, target=k, T=ref.random_pose(rng, 0.1, 0.2), info=ref.random_info(rng), uncertain=False) for k in range(5)]
    poses = np.stack(r3d.pipeline.poses_from_edges(edges))
    g = ref.Graph(poses, [(e["source"], e["target"]) for e in edges], [e["T"] for e in edges], [e["info"] for e in edges], [False] * 5)
    res = ref.global_optimization(g, dict(reference_node=0))
    assert res["trials"] == 0 and res["stops"] == (ref.STOP_RIGHT_TERM, ref.STOP_RIGHT_TERM) and g.poses.tobytes() == poses.tobytes()


def test_switches_and_limits():
    g, _ = ref.ring(6, closures=[(0, 3)], seed=2)
    base = ref.global_optimization(g.copy(), dict(reference_node=0), dict(max_iteration=5))
    for name in ("LAMBDA_SCALE_CAP_TWO_THIRDS", "X_NORM_EULER", "PRUNE_IN_LINE_PROCESS"):
        setattr(ref, name, True)
        try:
            other = ref.global_optimization(g.copy(), dict(reference_node=0), dict(max_iteration=5))
        finally:
            setattr(ref, name, False)
        assert other["trials"] >= 5 and np.isfinite(other["final"])
    assert base["trials"] >= 5
    assert ref.check_graph(g) is None and ref.check_graph(g, dict(reference_node=6)) and ref.check_graph(g, None, dict(max_iteration=-1))
    h = g.copy()
    h.nodes[0, 0] = h.nodes[0, 1]
    assert "itself" in ref.check_graph(h)
    empty = ref.Graph(g.poses[:1], np.zeros((0, 2)), np.zeros((0, 16)), np.zeros((0, 36)), [])
    res = ref.global_optimization(empty)
    assert res["trials"] == 0 and res["stops"] == (ref.STOP_NO_EDGES, ref.STOP_NO_EDGES) and np.array_equal(empty.poses, g.poses[:1])
    none = ref.global_optimization(g.copy(), None, dict(max_iteration_lm=0))
    assert none["trials"] == 0 and none["stops"][0] == ref.STOP_ITERATIONS


# ---- the package without a device ------------------------------------------------------------------------------------------------------
def test_json_round_trip_is_exact(r3d, tmp_path):
    g, _ = ref.ring(5, closures=[(0, 2)], seed=3)
    pg = r3d.posegraph
    graph = pg.PoseGraph([pg.PoseGraphNode(p) for p in g.poses],
                         [pg.PoseGraphEdge(int(s), int(t), T, L, bool(u), 0.1 + 0.2 * k) for k, ((s, t), T, L, u) in enumerate(zip(g.nodes, g.T, g.info, g.uncertain))])
    path = str(tmp_path / "graph.json")
    r3d.write_pose_graph(path, graph)
    back = r3d.read_pose_graph(path)
    assert len(back.nodes) == 5 and len(back.edges) == 6
    for a, b in zip(graph.nodes, back.nodes):
        assert a.pose.tobytes() == b.pose.tobytes()
    for a, b in zip(graph.edges, back.edges):
        assert (a.source_node_id, a.target_node_id, a.uncertain, a.confidence) == (b.source_node_id, b.target_node_id, b.uncertain, b.confidence)
        assert a.transformation.tobytes() == b.transformation.tobytes() and a.information.tobytes() == b.information.tobytes()
    import json
    doc = json.load(open(path))
    assert (doc["class_name"], doc["version_major"], doc["version_minor"]) == ("PoseGraph", 1, 0)
    assert doc["nodes"][1]["pose"][12:15] == list(g.poses[1][:3, 3]) and doc["edges"][0]["class_name"] == "PoseGraphEdge"     # column-major
    assert doc["edges"][2]["information"][1] == g.info[2][1, 0]


def test_python_refusals_need_no_device(r3d):
    pg = r3d.posegraph
    g, _ = ref.ring(4, seed=8)

    def code(**change):
        a = dict(poses=g.poses.copy(), nodes=g.nodes.copy(), T=g.T.copy(), info=g.info.copy(), uncertain=g.uncertain, confidence=None, params=None)
        a.update(change)
        with pytest.raises(r3d.R3DError) as e:
            pg.optimize(**a)
        return e.value.code
    bad_nodes, self_edge, nan_pose, inf_info = g.nodes.copy(), g.nodes.copy(), g.poses.copy(), g.info.copy()
    bad_nodes[1, 0], self_edge[2, 0], nan_pose[1, 0, 3], inf_info[0, 0, 0] = 4, self_edge[2, 1], np.nan, np.inf
    assert code(poses=np.zeros((0, 16))) == code(poses=np.tile(np.eye(4).reshape(1, 16), (1025, 1))) == -1
    assert code(nodes=bad_nodes) == code(nodes=self_edge) == code(poses=nan_pose) == code(info=inf_info) == code(T=g.T[:3]) == -1
    assert code(params=pg.posegraph_params(option=pg.GlobalOptimizationOption(reference_node=4))) == -1
    assert code(params=pg.posegraph_params(criteria=pg.GlobalOptimizationConvergenceCriteria(max_iteration=-1))) == -1
    with pytest.raises(r3d.R3DError) as e:
        r3d.global_optimization(pg.PoseGraph(), pg.GlobalOptimizationLevenbergMarquardt())
    assert e.value.code == -1
    with pytest.raises(r3d.R3DError) as e:
        r3d.global_optimization(pg.PoseGraph([pg.PoseGraphNode()]), object())
    assert e.value.code == -4


def test_graph_helpers(r3d):
    rng = np.random.default_rng(5)
    edges = [dict(source=k + 1, target=k, T=ref.random_pose(rng, 0.1, 0.2), info=ref.random_info(rng), uncertain=False) for k in range(3)]
    loop = dict(source=3, target=0, T=np.eye(4), info=np.eye(6), uncertain=True)
    graph = r3d.pipeline.pose_graph_from_edges(edges)
    assert [n.pose.tobytes() for n in graph.nodes] == [p.tobytes() for p in r3d.pipeline.poses_from_edges(edges)]
    assert [(e.source_node_id, e.target_node_id, e.uncertain, e.confidence) for e in graph.edges] == [(1, 0, False, 1.0), (2, 1, False, 1.0), (3, 2, False, 1.0)]
    with pytest.raises(ValueError):
        r3d.pipeline.pose_graph_from_edges(edges + [loop])                     # not a chain: the poses must be given
    both = r3d.pipeline.pose_graph_from_edges(edges + [loop], r3d.pipeline.poses_from_edges(edges))
    assert len(both.nodes) == 4 and both.edges[3].uncertain
    with pytest.raises(ValueError):
        r3d.pipeline.loop_closure_edges([], None, every=0)
    assert r3d.pipeline.loop_closure_edges([], None, every=5) == []
