"""numpy restatement of the pose-graph optimisation contract ("Pose-graph optimisation"), written from the
contract and not from the kernels.  [recalled, Open3D 0.18 pipelines/registration/GlobalOptimization.cpp, PoseGraph.h]: Open3D is
absent and the reference recorded no poses, so parity is UNPINNED; every choice memory leaves open is a named switch.

Everything is float64; a product and its addition are two roundings (no dot, matmul or einsum anywhere: BLAS fuses and reorders);
every sum starts from its first term and adds the others in ascending index unless stated.  A pose is a 4x4 camera-to-world matrix,
an edge's T maps source camera coordinates to target camera coordinates.

The contract is written twice: the *_loops functions are scalar loops, the others are vectorised and factor with the tiled
right-looking Cholesky; tests/test_posegraph_ref.py holds them bit-equal."""
import math

import numpy as np

f64 = np.float64

# ---- named switches ---------------------------------------------------------------------------------------------------------
# Open3D caps the factor that shrinks lambda after an accepted step at 2/3 [recalled]: scale = max(1/3, min(1 - (2 rho - 1)^3, 2/3)).
# Off (the library): scale = max(1/3, 1 - (2 rho - 1)^3).
LAMBDA_SCALE_CAP_TWO_THIRDS = False
# an uncertain edge's confidence is set to 0 once it falls below edge_prune_threshold, inside the line process [recalled, unsure].
# Off (the library): the confidence is kept as computed and the edge is only dropped between the two optimisations.
PRUNE_IN_LINE_PROCESS = False
# ||x|| of the relative-increment stop.  Open3D takes the norm of the 6-vectors TransformMatrix4dToVector6d(pose) (Euler angles by
# atan2).  Off (the library): the 6-vector of a pose is the one the residual uses, [(X21-X12)/2, (X02-X20)/2, (X10-X01)/2, X03, X13,
# X23], which needs no inverse trigonometric function; the two agree to first order and enter only a threshold scaled by 1e-6.
X_NORM_EULER = False

DEFAULT_OPTION = dict(max_correspondence_distance=0.03, edge_prune_threshold=0.25, preference_loop_closure=1.0, reference_node=-1)
DEFAULT_CRITERIA = dict(max_iteration=100, min_relative_increment=1e-6, min_relative_residual_increment=1e-6, min_right_term=1e-6,
                        min_residual=1e-6, max_iteration_lm=20, upper_scale_factor=2.0 / 3.0, lower_scale_factor=1.0 / 3.0)
MAX_NODES, MAX_EDGES = 1024, 1 << 20
ANGLE_LIMIT = 2.0 ** 30        # an angle at or beyond it (or not finite) gives NaN: the trial is then rejected

# trace codes of a trial that never reached rho
TRIAL_REJECTED, TRIAL_ACCEPTED, TRIAL_SMALL_STEP, TRIAL_FACTOR_FAILED = 0.0, 1.0, -1.0, -2.0
# why an optimisation stopped
STOP_NONE, STOP_RIGHT_TERM, STOP_INCREMENT, STOP_RESIDUAL_INCREMENT, STOP_RESIDUAL, STOP_ITERATIONS, STOP_NO_EDGES = 0, 1, 2, 3, 4, 5, 6


# ---- sine and cosine: the contract's own, because libm's and the device library's need not agree in the last bit ---------------
# k = rint(x * 2/pi); r = ((x - k P1) - k P2) - k P3 (Cody-Waite, fdlibm's three parts of pi/2); Taylor polynomials in r^2 by Horner,
# sin r = r + r (r^2 S), cos r = 1 + r^2 C; the quadrant k mod 4 picks and signs them.  Within 2 ulp of the exact value for
# |x| < 1e5 (tests/test_posegraph_ref.py measures it against numpy).
TWO_OVER_PI = 6.36619772367581382433e-01
PIO2_1, PIO2_2, PIO2_3 = 1.57079632673412561417e+00, 6.07710050650619224932e-11, 2.02226624879595063154e-21
SIN_C = [-1.0 / 6.0, 1.0 / 120.0, -1.0 / 5040.0, 1.0 / 362880.0, -1.0 / 39916800.0, 1.0 / 6227020800.0, -1.0 / 1307674368000.0,
         1.0 / 355687428096000.0, -1.0 / 121645100408832000.0]
COS_C = [-1.0 / 2.0, 1.0 / 24.0, -1.0 / 720.0, 1.0 / 40320.0, -1.0 / 3628800.0, 1.0 / 479001600.0, -1.0 / 87178291200.0,
         1.0 / 20922789888000.0, -1.0 / 6402373705728000.0]


def sincos(x):
    """-> (sin x, cos x) of an array, by the contract's own evaluation"""
    x = np.asarray(x, dtype=f64)
    with np.errstate(all="ignore"):
        bad = ~(np.abs(x) < ANGLE_LIMIT)
        xs = np.where(bad, 0.0, x)
        k = np.rint(xs * TWO_OVER_PI)
        r = ((xs - k * PIO2_1) - k * PIO2_2) - k * PIO2_3
        z = r * r
        ps = np.full_like(z, SIN_C[-1])
        pc = np.full_like(z, COS_C[-1])
        for c in SIN_C[-2::-1]:
            ps = ps * z + c
        for c in COS_C[-2::-1]:
            pc = pc * z + c
        s = r + r * (z * ps)
        c = 1.0 + z * pc
        q = k.astype(np.int64) & 3
        sn = np.where(q == 0, s, np.where(q == 1, c, np.where(q == 2, -s, -c)))
        cs = np.where(q == 0, c, np.where(q == 1, -s, np.where(q == 2, -c, s)))
        return np.where(bad, np.nan, sn), np.where(bad, np.nan, cs)


def sincos_loops(x):
    x = float(x)
    if not abs(x) < ANGLE_LIMIT:
        return float("nan"), float("nan")
    k = float(np.rint(f64(x * TWO_OVER_PI)))
    r = ((x - k * PIO2_1) - k * PIO2_2) - k * PIO2_3
    z = r * r
    ps, pc = SIN_C[-1], COS_C[-1]
    for c in SIN_C[-2::-1]:
        ps = ps * z + c
    for c in COS_C[-2::-1]:
        pc = pc * z + c
    s = r + r * (z * ps)
    c = 1.0 + z * pc
    q = int(k) & 3
    return [(s, c), (c, -s), (-s, -c), (-c, s)][q]


# ---- 4x4 algebra ------------------------------------------------------------------------------------------------------------
def mul4(A, B):
    """C[i][j] = ((A[i][0] B[0][j] + A[i][1] B[1][j]) + A[i][2] B[2][j]) + A[i][3] B[3][j]; arrays [..., 4, 4]"""
    A, B = np.asarray(A, dtype=f64), np.asarray(B, dtype=f64)
    with np.errstate(all="ignore"):
        return ((A[..., :, 0:1] * B[..., 0:1, :] + A[..., :, 1:2] * B[..., 1:2, :]) + A[..., :, 2:3] * B[..., 2:3, :]) + A[..., :, 3:4] * B[..., 3:4, :]


def mul4_loops(A, B):
    C = [[0.0] * 4 for _ in range(4)]
    for i in range(4):
        for j in range(4):
            C[i][j] = ((A[i][0] * B[0][j] + A[i][1] * B[1][j]) + A[i][2] * B[2][j]) + A[i][3] * B[3][j]
    return C


def inv_rigid(X):
    """[R t; 0 1] -> [R' -R't; 0 1], (R't)[a] = (R[0][a] t0 + R[1][a] t1) + R[2][a] t2; the last row of X is not read"""
    X = np.asarray(X, dtype=f64)
    out = np.zeros_like(X)
    out[..., :3, :3] = np.swapaxes(X[..., :3, :3], -1, -2)
    t = X[..., :3, 3]
    for a in range(3):
        out[..., a, 3] = -((X[..., 0, a] * t[..., 0] + X[..., 1, a] * t[..., 1]) + X[..., 2, a] * t[..., 2])
    out[..., 3, 3] = 1.0
    return out


def inv_rigid_loops(X):
    out = [[0.0] * 4 for _ in range(4)]
    for a in range(3):
        for c in range(3):
            out[a][c] = X[c][a]
        out[a][3] = -((X[0][a] * X[0][3] + X[1][a] * X[1][3]) + X[2][a] * X[2][3])
    out[3][3] = 1.0
    return out


def _generators():
    G = np.zeros((6, 4, 4), f64)
    G[0, 1, 2], G[0, 2, 1] = -1.0, 1.0
    G[1, 0, 2], G[1, 2, 0] = 1.0, -1.0
    G[2, 0, 1], G[2, 1, 0] = -1.0, 1.0
    for k in range(3):
        G[3 + k, k, 3] = 1.0
    return G


GENERATORS = _generators()


def vec6(M):
    """[(M21 - M12) / 2, (M02 - M20) / 2, (M10 - M01) / 2, M03, M13, M23] of arrays [..., 4, 4] -> [..., 6]"""
    M = np.asarray(M, dtype=f64)
    return np.stack([(M[..., 2, 1] - M[..., 1, 2]) * 0.5, (M[..., 0, 2] - M[..., 2, 0]) * 0.5, (M[..., 1, 0] - M[..., 0, 1]) * 0.5,
                     M[..., 0, 3], M[..., 1, 3], M[..., 2, 3]], -1)


def vec6_loops(M):
    return [(M[2][1] - M[1][2]) * 0.5, (M[0][2] - M[2][0]) * 0.5, (M[1][0] - M[0][1]) * 0.5, M[0][3], M[1][3], M[2][3]]


def exp6(d):
    """TransformVector6dToMatrix4d: R = Rz(d2) Ry(d1) Rx(d0), t = d[3:6]; arrays [..., 6] -> [..., 4, 4]"""
    d = np.asarray(d, dtype=f64)
    (sa, ca), (sb, cb), (sc, cc) = sincos(d[..., 0]), sincos(d[..., 1]), sincos(d[..., 2])
    U = np.zeros(d.shape[:-1] + (4, 4), f64)
    with np.errstate(all="ignore"):
        U[..., 0, 0], U[..., 0, 1], U[..., 0, 2] = cc * cb, cc * sb * sa - sc * ca, cc * sb * ca + sc * sa
        U[..., 1, 0], U[..., 1, 1], U[..., 1, 2] = sc * cb, sc * sb * sa + cc * ca, sc * sb * ca - cc * sa
        U[..., 2, 0], U[..., 2, 1], U[..., 2, 2] = -sb, cb * sa, cb * ca
    U[..., :3, 3] = d[..., 3:6]
    U[..., 3, 3] = 1.0
    return U


def exp6_loops(d):
    (sa, ca), (sb, cb), (sc, cc) = sincos_loops(d[0]), sincos_loops(d[1]), sincos_loops(d[2])
    return [[cc * cb, cc * sb * sa - sc * ca, cc * sb * ca + sc * sa, d[3]], [sc * cb, sc * sb * sa + cc * ca, sc * sb * ca - cc * sa, d[4]],
            [-sb, cb * sa, cb * ca, d[5]], [0.0, 0.0, 0.0, 1.0]]


def _seq(terms, axis=0):
    """sum along an axis, first term first, one addition at a time (np.sum adds pairwise)"""
    t = np.moveaxis(np.asarray(terms, dtype=f64), axis, 0)
    acc = t[0].copy()
    with np.errstate(all="ignore"):
        for q in range(1, t.shape[0]):
            acc = acc + t[q]
    return acc


# ---- graph ------------------------------------------------------------------------------------------------------------------
class Graph:
    """arrays of a pose graph: poses [N,4,4]; nodes [E,2] (source, target); T [E,4,4]; info [E,6,6]; uncertain [E] bool;
    confidence [E]; kept [E] bool"""

    def __init__(self, poses, nodes, T, info, uncertain, confidence=None, kept=None):
        self.poses = np.array(poses, dtype=f64).reshape(-1, 4, 4)
        self.nodes = np.array(nodes, dtype=np.int32).reshape(-1, 2)
        E = len(self.nodes)
        self.T = np.array(T, dtype=f64).reshape(E, 4, 4)
        self.info = np.array(info, dtype=f64).reshape(E, 6, 6)
        self.uncertain = np.array(uncertain, dtype=bool).reshape(E)
        self.confidence = np.ones(E, f64) if confidence is None else np.array(confidence, dtype=f64).reshape(E)
        self.kept = np.ones(E, bool) if kept is None else np.array(kept, dtype=bool).reshape(E)

    def copy(self):
        return Graph(self.poses, self.nodes, self.T, self.info, self.uncertain, self.confidence, self.kept)


def check_graph(g, option=None, criteria=None):
    """the refusals of the library (R3D_E_BADARG) -> None or a message"""
    o, c = dict(DEFAULT_OPTION, **(option or {})), dict(DEFAULT_CRITERIA, **(criteria or {}))
    N, E = len(g.poses), len(g.nodes)
    if N < 1 or N > MAX_NODES:
        return "node count outside 1..1024"
    if E > MAX_EDGES:
        return "more than 2^20 edges"
    if E and (g.nodes.min() < 0 or g.nodes.max() >= N):
        return "node id out of range"
    if E and (g.nodes[:, 0] == g.nodes[:, 1]).any():
        return "an edge joins a node to itself"
    if not (np.isfinite(g.poses).all() and np.isfinite(g.T).all() and np.isfinite(g.info).all() and np.isfinite(g.confidence).all()):
        return "a non-finite pose, transformation, information matrix or confidence"
    if not -1 <= o["reference_node"] < N:
        return "reference_node out of range"
    if c["max_iteration"] < 0 or c["max_iteration_lm"] < 0:
        return "negative iteration count"
    return None


def line_process_mu(g, option):
    """mu = ((preference_loop_closure * mcd) * mcd) * (sum of info[5][5] over the kept edges, ascending / their number); 0 with none"""
    idx = np.flatnonzero(g.kept)
    if len(idx) == 0:
        return 0.0
    mean = float(_seq(g.info[idx, 5, 5])) / float(len(idx))
    return float(((f64(option["preference_loop_closure"]) * f64(option["max_correspondence_distance"])) * f64(option["max_correspondence_distance"])) * f64(mean))


def edge_terms(g, poses=None):
    """per edge: e [E,6], J_s [E,6,6] (J[p][k] = component p of column k), Le = info e, q = e' info e, W = J' (info J), gr = J' (info e)"""
    X = g.poses if poses is None else poses
    s, t = g.nodes[:, 0], g.nodes[:, 1]
    P = mul4(inv_rigid(g.T), inv_rigid(X[t]))
    Xs = X[s]
    e = vec6(mul4(P, Xs))
    J = np.stack([vec6(mul4(P, mul4(GENERATORS[k], Xs))) for k in range(6)], -1)
    L = g.info
    with np.errstate(all="ignore"):
        Le = _seq(L * e[:, None, :], axis=2)                                     # [E,6]: sum over q of L[p][q] e[q]
        q = _seq(e * Le, axis=1)
        LJ = _seq(L[:, :, :, None] * J[:, None, :, :], axis=2)                   # [E,p,c]: sum over q of L[p][q] J[q][c]
        W = _seq(J[:, :, :, None] * LJ[:, :, None, :], axis=1)                   # [E,a,c]: sum over p of J[p][a] LJ[p][c]
        gr = _seq(J * Le[:, :, None], axis=1)                                    # [E,a]: sum over p of J[p][a] Le[p]
    return e, J, Le, q, W, gr


def edge_terms_loops(g, k, poses=None):
    """edge_terms for edge k, scalar loops -> e, J, q, W, gr as nested lists"""
    X = g.poses if poses is None else poses
    s, t = int(g.nodes[k, 0]), int(g.nodes[k, 1])
    P = mul4_loops(inv_rigid_loops(g.T[k].tolist()), inv_rigid_loops(X[t].tolist()))
    Xs = X[s].tolist()
    e = vec6_loops(mul4_loops(P, Xs))
    cols = [vec6_loops(mul4_loops(P, mul4_loops(GENERATORS[c].tolist(), Xs))) for c in range(6)]
    J = [[cols[c][p] for c in range(6)] for p in range(6)]
    L = g.info[k].tolist()

    def dot(terms):
        acc = terms[0]
        for v in terms[1:]:
            acc = acc + v
        return acc
    Le = [dot([L[p][q] * e[q] for q in range(6)]) for p in range(6)]
    q = dot([e[p] * Le[p] for p in range(6)])
    LJ = [[dot([L[p][q_] * J[q_][c] for q_ in range(6)]) for c in range(6)] for p in range(6)]
    W = [[dot([J[p][a] * LJ[p][c] for p in range(6)]) for c in range(6)] for a in range(6)]
    gr = [dot([J[p][a] * Le[p] for p in range(6)]) for a in range(6)]
    return e, J, q, W, gr


def weights(g):
    """l per edge: 1 for a certain edge, the stored confidence for an uncertain one"""
    return np.where(g.uncertain, g.confidence, 1.0)


def line_process(g, q, mu, option):
    """the confidences of the uncertain kept edges from their q = e' info e: (mu / (mu + q))^2"""
    with np.errstate(all="ignore"):
        r = mu / (mu + q)
        c = r * r
    if PRUNE_IN_LINE_PROCESS:
        c = np.where(c < option["edge_prune_threshold"], 0.0, c)
    return np.where(g.uncertain & g.kept, c, g.confidence)


def objective(g, q, l, mu):
    """F = (sum over kept edges of l q, ascending) + (sum over uncertain kept edges of mu ((sqrt l - 1) (sqrt l - 1)), ascending)"""
    F1, F2 = 0.0, 0.0
    with np.errstate(all="ignore"):
        a = l * q
        d = np.sqrt(l) - 1.0
        p = mu * (d * d)
    for k in range(len(q)):
        if g.kept[k]:
            F1 = F1 + float(a[k])
            if g.uncertain[k]:
                F2 = F2 + float(p[k])
    return F1 + F2


def linearize(g, poses=None):
    """-> e [E,6], l [E], H [6N,6N], b [6N], q [E].  Contributions in ascending edge index over the kept edges.  With Wl = l W:
    block (s,s) += Wl, (t,t) += Wl, and of the blocks between s and t the one BELOW the diagonal -= Wl (s > t) or -= Wl' (s < t);
    b_s += l gr, b_t -= l gr.  Only the lower triangle of H is built; the upper one is its mirror image."""
    N = len(g.poses)
    e, J, Le, q, W, gr = edge_terms(g, poses)
    l = weights(g)
    H, b = np.zeros((6 * N, 6 * N), f64), np.zeros(6 * N, f64)
    with np.errstate(all="ignore"):
        Wl, gl = l[:, None, None] * W, l[:, None] * gr
    for k in range(len(g.nodes)):
        if not g.kept[k]:
            continue
        s, t = 6 * int(g.nodes[k, 0]), 6 * int(g.nodes[k, 1])
        H[s:s + 6, s:s + 6] += Wl[k]
        H[t:t + 6, t:t + 6] += Wl[k]
        if s > t:
            H[s:s + 6, t:t + 6] -= Wl[k]
        else:
            H[t:t + 6, s:s + 6] -= Wl[k].T
        b[s:s + 6] += gl[k]
        b[t:t + 6] -= gl[k]
    H = np.tril(H) + np.tril(H, -1).T
    return e, l, H, b, q


def linearize_loops(g, poses=None):
    N, E = len(g.poses), len(g.nodes)
    H = [[0.0] * (6 * N) for _ in range(6 * N)]
    b = [0.0] * (6 * N)
    es, qs = [], []
    l = weights(g).tolist()
    for k in range(E):
        e, J, q, W, gr = edge_terms_loops(g, k, poses)
        es.append(e)
        qs.append(q)
        if not g.kept[k]:
            continue
        s, t = 6 * int(g.nodes[k, 0]), 6 * int(g.nodes[k, 1])
        for a in range(6):
            for c in range(6):
                w = l[k] * W[a][c]
                if c <= a:
                    H[s + a][s + c] = H[s + a][s + c] + w
                    H[t + a][t + c] = H[t + a][t + c] + w
                if s > t:
                    H[s + a][t + c] = H[s + a][t + c] - w
                else:
                    H[t + c][s + a] = H[t + c][s + a] - w
            b[s + a] = b[s + a] + l[k] * gr[a]
            b[t + a] = b[t + a] - l[k] * gr[a]
    H = np.array(H, dtype=f64).reshape(6 * N, 6 * N)
    H = np.tril(H) + np.tril(H, -1).T
    return np.array(es, dtype=f64).reshape(E, 6), np.array(l, dtype=f64), H, np.array(b, dtype=f64), np.array(qs, dtype=f64)


# ---- the solve --------------------------------------------------------------------------------------------------------------
def cholesky_loops(A):
    """L[i][j] = (A[i][j] - sum_{k<j} L[i][k] L[j][k]) / L[j][j], k ascending, one product and one subtraction at a time; L[j][j] the
    square root of the same expression.  Columns in ascending j.  A pivot <= 0 or not finite stops: -> (L with the columns from
    that one on zero, its index), else (L, -1).  Reads the lower triangle only; the strict upper triangle of L is zero."""
    n = len(A)
    L = [[0.0] * n for _ in range(n)]
    for j in range(n):
        v = float(A[j][j])
        for k in range(j):
            v = v - L[j][k] * L[j][k]
        if not (v > 0.0 and math.isfinite(v)):
            return np.array(L, dtype=f64).reshape(n, n), j
        d = math.sqrt(v)
        L[j][j] = d
        for i in range(j + 1, n):
            v = float(A[i][j])
            for k in range(j):
                v = v - L[i][k] * L[j][k]
            L[i][j] = v / d
    return np.array(L, dtype=f64).reshape(n, n), -1


def cholesky_columns(A):
    """the same, the loop over i vectorised (left-looking)"""
    A = np.asarray(A, dtype=f64)
    n = len(A)
    L = np.zeros((n, n), f64)
    with np.errstate(all="ignore"):
        for j in range(n):
            v = A[j:, j].copy()
            for k in range(j):
                v = v - L[j:, k] * L[j, k]
            if not (v[0] > 0.0 and np.isfinite(v[0])):
                return L, j
            d = np.sqrt(v[0])
            L[j:, j] = v / d
            L[j, j] = d
    return L, -1


def cholesky_tiled(A, tile=64):
    """the same entries by a right-looking tiled factorisation: per panel of `tile` columns the diagonal tile, the rows below it,
    then the trailing lower triangle tile by tile, each entry taking the panel's products in ascending k.  Every entry sees its
    products in ascending k over the whole factorisation, so the tile does not show in the result."""
    W = np.tril(np.asarray(A, dtype=f64))
    n = len(W)
    with np.errstate(all="ignore"):
        for p0 in range(0, n, tile):
            p1 = min(n, p0 + tile)
            for j in range(p0, p1):
                v = W[j, j]
                if not (v > 0.0 and np.isfinite(v)):
                    W[:, j:] = 0.0
                    return np.tril(W), j
                d = np.sqrt(v)
                W[j + 1:, j] = W[j + 1:, j] / d
                W[j, j] = d
                if j + 1 < p1:                                       # the panel's later columns take column j
                    W[j + 1:, j + 1:p1] -= W[j + 1:, j:j + 1] * W[j + 1:p1, j][None, :]
            for i0 in range(p1, n, tile):
                i1 = min(n, i0 + tile)
                for j0 in range(p1, i1, tile):
                    j1 = min(n, j0 + tile)
                    blk = W[i0:i1, j0:j1]
                    for k in range(p0, p1):
                        blk -= W[i0:i1, k:k + 1] * W[j0:j1, k][None, :]
    return np.tril(W), -1


def substitute_loops(L, c):
    """forward: y[i] = (c[i] - sum_{k<i} L[i][k] y[k]) / L[i][i], k ascending; back: x[i] = (y[i] - sum_{k>i} L[k][i] x[k]) / L[i][i],
    k DESCENDING from n - 1"""
    n = len(c)
    y = [0.0] * n
    for i in range(n):
        v = float(c[i])
        for k in range(i):
            v = v - float(L[i][k]) * y[k]
        y[i] = v / float(L[i][i])
    x = [0.0] * n
    for i in range(n - 1, -1, -1):
        v = y[i]
        for k in range(n - 1, i, -1):
            v = v - float(L[k][i]) * x[k]
        x[i] = v / float(L[i][i])
    return np.array(x, dtype=f64)


def substitute(L, c):
    """the same, right-looking: a solved unknown is taken out of every later one at once"""
    L = np.asarray(L, dtype=f64)
    n = len(c)
    y = np.array(c, dtype=f64)
    with np.errstate(all="ignore"):
        for k in range(n):
            y[k] = y[k] / L[k, k]
            y[k + 1:] -= L[k + 1:, k] * y[k]
        for k in range(n - 1, -1, -1):
            y[k] = y[k] / L[k, k]
            y[:k] -= L[k, :k] * y[k]
    return y


def solve(A, b, lam, tile=64, how="tiled"):
    """(A + lam I) delta = -b -> L, delta, failed pivot or -1.  On a failed pivot L and delta are all zero (what the library hands
    out: nothing past the failure is worth reading)."""
    A = np.array(A, dtype=f64)
    n = len(A)
    A[np.arange(n), np.arange(n)] = A[np.arange(n), np.arange(n)] + f64(lam)
    L, fail = {"tiled": lambda: cholesky_tiled(A, tile), "columns": lambda: cholesky_columns(A), "loops": lambda: cholesky_loops(A)}[how]()
    if fail >= 0:
        return np.zeros((n, n), f64), np.zeros(n, f64), fail
    c = -np.asarray(b, dtype=f64)
    return L, (substitute_loops(L, c) if how == "loops" else substitute(L, c)), -1


# ---- Levenberg-Marquardt ----------------------------------------------------------------------------------------------------
def pose_vector_norm(poses):
    v = vec6(poses).reshape(-1)
    if X_NORM_EULER:
        R = poses[:, :3, :3]
        sy = np.sqrt(R[:, 0, 0] * R[:, 0, 0] + R[:, 1, 0] * R[:, 1, 0])
        v = np.stack([np.arctan2(R[:, 2, 1], R[:, 2, 2]), np.arctan2(-R[:, 2, 0], sy), np.arctan2(R[:, 1, 0], R[:, 0, 0]),
                      poses[:, 0, 3], poses[:, 1, 3], poses[:, 2, 3]], -1).reshape(-1)
    with np.errstate(all="ignore"):
        return float(np.sqrt(_seq(v * v)))


def optimize(g, option=None, criteria=None, how="tiled", tile=64):
    """One Levenberg-Marquardt optimisation of the kept edges of g, in place (poses, confidence).  -> dict(outer, trials, rejected,
    failed, first, final, stop, trace [trials,4] of (lambda, F_new, rho, code)).

    State: lambda, nu = 2, F.  An outer iteration is up to max_iteration_lm trials and ends with the first accepted one; the
    optimisation ends after max_iteration outer iterations or at a stop.  A trial:
      1. (H + lambda I) delta = -b by Cholesky; a failed pivot: code -2, counted as rejected and as a failed factorisation,
         lambda *= nu, nu *= 2.
      2. the six entries of reference_node are zeroed; ||delta|| < min_relative_increment (||x|| + min_relative_increment): code -1,
         poses untouched, stop.
      3. X_i <- exp6(delta_i) X_i on a copy; F_new = the objective there with the CURRENT weights l;
         rho = (F - F_new) / (sum_i delta_i (lambda delta_i - b_i) + 1e-3).
      4. rho > 0: the copy becomes the poses, lambda *= max(1/3, 1 - (2 rho - 1)^3), nu = 2; the confidences of the uncertain edges
         are recomputed there, H, b and F follow from the new poses and weights; then the stops, in this order: F_old - F_new <
         min_relative_residual_increment F_old; F_new < min_residual; max|b| < min_right_term.
         otherwise (NaN included): lambda *= nu, nu *= 2."""
    o, c = dict(DEFAULT_OPTION, **(option or {})), dict(DEFAULT_CRITERIA, **(criteria or {}))
    lin = linearize_loops if how == "loops" else linearize
    N = len(g.poses)
    ref = int(o["reference_node"])
    res = dict(outer=0, trials=0, rejected=0, failed=0, first=0.0, final=0.0, stop=STOP_NONE, trace=[])
    if not g.kept.any():
        res["stop"] = STOP_NO_EDGES
        res["trace"] = np.zeros((0, 4), f64)
        return res
    mu = line_process_mu(g, o)
    e, l, H, b, q = lin(g)
    F = objective(g, q, l, mu)
    res["first"] = res["final"] = F
    lam, nu = 1e-5 * float(np.max(np.diag(H))), 2.0
    if float(np.max(np.abs(b))) < c["min_right_term"]:
        res["stop"] = STOP_RIGHT_TERM
    inner = 0
    if c["max_iteration"] == 0 or c["max_iteration_lm"] == 0:
        res["stop"] = res["stop"] or STOP_ITERATIONS
    with np.errstate(all="ignore"):
        while res["stop"] == STOP_NONE:
            res["trials"] += 1
            inner += 1
            accepted = False
            _, delta, fail = solve(H, b, lam, tile=tile, how=how)
            if fail >= 0:
                res["failed"] += 1
                res["rejected"] += 1
                res["trace"].append([lam, 0.0, 0.0, TRIAL_FACTOR_FAILED])
                lam, nu = lam * nu, nu * 2.0
            else:
                if ref >= 0:
                    delta[6 * ref:6 * ref + 6] = 0.0
                dn = float(np.sqrt(_seq(delta * delta)))
                if dn < c["min_relative_increment"] * (pose_vector_norm(g.poses) + c["min_relative_increment"]):
                    res["trace"].append([lam, 0.0, 0.0, TRIAL_SMALL_STEP])
                    res["stop"] = STOP_INCREMENT
                    break
                trial = mul4(exp6(delta.reshape(N, 6)), g.poses)
                q_new = edge_terms(g, trial)[3] if how != "loops" else np.array([edge_terms_loops(g, k, trial)[2] for k in range(len(g.nodes))])
                F_new = objective(g, q_new, l, mu)
                den = float(_seq(delta * (lam * delta - b))) + 1e-3
                rho = (F - F_new) / den
                if rho > 0:
                    accepted = True
                    res["trace"].append([lam, F_new, rho, TRIAL_ACCEPTED])
                    t = 2.0 * rho - 1.0
                    scale = 1.0 - (t * t) * t
                    if LAMBDA_SCALE_CAP_TWO_THIRDS:
                        scale = min(scale, 2.0 / 3.0)
                    lam, nu = lam * max(1.0 / 3.0, scale), 2.0
                    g.poses = trial
                    g.confidence = line_process(g, q_new, mu, o)
                    e, l, H, b, q = lin(g)
                    F_old, F = F, objective(g, q, l, mu)
                    res["final"] = F
                    if F_old - F_new < c["min_relative_residual_increment"] * F_old:
                        res["stop"] = STOP_RESIDUAL_INCREMENT
                    elif F_new < c["min_residual"]:
                        res["stop"] = STOP_RESIDUAL
                    elif float(np.max(np.abs(b))) < c["min_right_term"]:
                        res["stop"] = STOP_RIGHT_TERM
                else:
                    res["rejected"] += 1
                    res["trace"].append([lam, F_new, rho, TRIAL_REJECTED])
                    lam, nu = lam * nu, nu * 2.0
            if accepted or inner >= c["max_iteration_lm"]:
                res["outer"] += 1
                inner = 0
                if res["outer"] >= c["max_iteration"] and res["stop"] == STOP_NONE:
                    res["stop"] = STOP_ITERATIONS
    res["trace"] = np.array(res["trace"], dtype=f64).reshape(-1, 4)
    return res


def global_optimization(g, option=None, criteria=None, how="tiled", tile=64):
    """optimise; drop the uncertain edges whose confidence is below edge_prune_threshold; optimise the rest; if the reference
    node's pose changed (it cannot while its six entries are zeroed, short of a NaN), left-multiply every pose by
    X_ref_before inv_rigid(X_ref_after).  In place.  -> dict(outer, trials, rejected, failed, pruned, first, final, stops, trace)"""
    o = dict(DEFAULT_OPTION, **(option or {}))
    bad = check_graph(g, option, criteria)
    if bad:
        raise ValueError(bad)
    ref = int(o["reference_node"])
    before = g.poses[ref].copy() if ref >= 0 else None
    g.kept = np.ones(len(g.nodes), bool)
    r1 = optimize(g, option, criteria, how, tile)
    g.kept = ~(g.uncertain & (g.confidence < o["edge_prune_threshold"]))
    r2 = optimize(g, option, criteria, how, tile)
    if ref >= 0 and not np.array_equal(before, g.poses[ref]):
        g.poses = mul4(mul4(before, inv_rigid(g.poses[ref]))[None], g.poses)
    return dict(outer=r1["outer"] + r2["outer"], trials=r1["trials"] + r2["trials"], rejected=r1["rejected"] + r2["rejected"],
                failed=r1["failed"] + r2["failed"], pruned=int((~g.kept).sum()), first=r1["first"], final=r2["final"] if g.kept.any() else r1["final"],
                stops=(r1["stop"], r2["stop"]), trace=np.concatenate([r1["trace"], r2["trace"]]))


# ---- test graphs ------------------------------------------------------------------------------------------------------------
def random_pose(rng, angle=0.3, shift=1.0):
    return exp6(np.concatenate([rng.uniform(-angle, angle, 3), rng.uniform(-shift, shift, 3)]))


def random_info(rng):
    B = rng.normal(size=(6, 6))
    A = B @ B.T + 6.0 * np.eye(6)
    return (A + A.T) * 0.5 * 100.0


def ring(n, closures=(), wrong=None, noise=0.02, seed=0):
    """n poses on a circle looking along it; odometry edges k+1 -> k and the edge 0 -> n-1 from the truth (certain), `closures`
    (s, t) pairs from the truth (uncertain), the pair `wrong` with 0.5 m added to its translation; node poses perturbed by noise.
    -> Graph, truth [n,4,4]"""
    rng = np.random.default_rng(seed)
    truth = np.stack([exp6(np.array([0.0, 0.0, 2 * np.pi * k / n, np.cos(2 * np.pi * k / n), np.sin(2 * np.pi * k / n), 0.1 * k])) for k in range(n)])
    pairs = [(k + 1, k, False) for k in range(n - 1)] + [(0, n - 1, False)] + [(s, t, True) for s, t in closures]
    T = []
    for s, t, _ in pairs:
        M = np.linalg.inv(truth[t]) @ truth[s]
        if wrong is not None and (s, t) == tuple(wrong):
            M = M.copy()
            M[0, 3] += 0.5
        T.append(M)
    poses = np.stack([mul4(exp6(rng.normal(scale=noise, size=6)), truth[k]) for k in range(n)])
    poses[0] = truth[0]
    info = np.stack([random_info(rng) for _ in pairs])
    return Graph(poses, [(s, t) for s, t, _ in pairs], T, info, [u for _, _, u in pairs]), truth


def random_graph(n, E, seed=0, hub=True):
    """E random edges among n nodes with noisy T; with hub, a tenth of the nodes take most of the edges (degrees differ by > 10x)"""
    rng = np.random.default_rng(seed)
    truth = np.stack([random_pose(rng) for _ in range(n)])
    hubs = max(1, n // 10)
    nodes = []
    while len(nodes) < E:
        s = int(rng.integers(0, hubs)) if hub and rng.random() < 0.7 else int(rng.integers(0, n))
        t = int(rng.integers(0, n))
        if s != t:
            nodes.append((s, t) if rng.random() < 0.5 else (t, s))
    T = np.stack([mul4(exp6(rng.normal(scale=0.01, size=6)), np.linalg.inv(truth[t]) @ truth[s]) for s, t in nodes])
    info = np.stack([random_info(rng) for _ in nodes])
    unc = rng.random(E) < 0.4
    conf = np.where(unc, rng.uniform(0.1, 1.0, E), 1.0)
    poses = np.stack([mul4(exp6(rng.normal(scale=0.02, size=6)), truth[k]) for k in range(n)])
    return Graph(poses, nodes, T, info, unc, conf)


def spd(n, seed=0):
    """a symmetric positive definite matrix of order n with a condition number in the hundreds, and a right-hand side"""
    rng = np.random.default_rng(seed)
    B = rng.normal(size=(n, n)) / np.sqrt(n)
    A = B @ B.T
    A = (A + A.T) * 0.5 + 0.05 * np.eye(n)
    return A, rng.normal(size=n)
