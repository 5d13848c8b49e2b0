"""numpy restatement of Open3D's coloured ICP (registration_colored_icp; Park, Zhou, Koltun 2017), written from the contract in
DESIGN.md section 4, "Coloured ICP" [recalled, Open3D 0.18 pipelines/registration/ColoredICP.cpp; nothing here can pin it],
not from the HIP kernels.  The neighbour search, the 1-NN evaluation, the 6x6 solve and the pose arithmetic are the oracle's, so the search order
(squared distance, index) and the loop around ComputeTransformation are those of oracle.cloud_oracle.registration.

Switches (each names a choice the original leaves open or that was restated from memory):
  QUIRK_SINGULAR  a gradient system whose determinant is zero, below 1e-300 or not finite, or whose solution is not finite, gives
                  a ZERO gradient.  The original calls Eigen's LDLT and uses whatever comes out.
"""
import numpy as np
from scipy.spatial import cKDTree

from oracle import cloud_oracle as co

QUIRK_SINGULAR = True
LAMBDA_GEOMETRIC = 0.968


def intensity(colors, dtype=np.float64):
    c = np.asarray(colors, dtype)
    return ((c[:, 0] + c[:, 1]) + c[:, 2]) / dtype(3)


def _inv3_sym(m):
    """Inverse of symmetric 3x3 matrices given as [n,6] (xx xy xz yy yz zz) by cofactors, in m's own dtype (numpy's LAPACK
    routines have no extended precision).  Returns (inverse [n,6], determinant [n])."""
    c00 = m[:, 3] * m[:, 5] - m[:, 4] * m[:, 4]
    c01 = m[:, 2] * m[:, 4] - m[:, 1] * m[:, 5]
    c02 = m[:, 1] * m[:, 4] - m[:, 2] * m[:, 3]
    det = m[:, 0] * c00 + m[:, 1] * c01 + m[:, 2] * c02
    with np.errstate(all="ignore"):
        idet = 1 / det
        inv = np.stack([c00 * idet, c01 * idet, c02 * idet, (m[:, 0] * m[:, 5] - m[:, 2] * m[:, 2]) * idet,
                        (m[:, 1] * m[:, 2] - m[:, 0] * m[:, 4]) * idet, (m[:, 0] * m[:, 3] - m[:, 1] * m[:, 1]) * idet], 1)
    return inv, det


def color_gradients(points, normals, colors, radius, max_nn=30, dtype=np.float64, neighbors=None):
    """InitializePointCloudForColoredICP.  Returns (intensity [n], gradient [n,3], neighbour count [n]) in `dtype`.
    Point k with position v, normal n, intensity I_v and hybrid neighbours p_0 (itself), p_1 .. p_(nn-1), nearest first:
    rows A[i-1] = (p_i - ((p_i - v).n) n) - v, b[i-1] = I_i - I_v for i = 1 .. nn-1, a last row (nn-1) n with b = 0;
    gradient = (A^T A)^-1 A^T b, the normal equations summed in neighbour order; 0 when nn < 4.
    `neighbors`: the lists of co.hybrid_neighbors(points, radius, max_nn), to share one search between precisions."""
    P = np.asarray(points, np.float64)
    nb = co.hybrid_neighbors(P, radius, max_nn) if neighbors is None else neighbors
    n = len(P)
    cnt = np.fromiter((len(x) for x in nb), np.int64, n)
    kmax = int(cnt.max()) if n else 0
    pad = np.zeros((n, max(kmax, 1)), np.int64)
    for i, ix in enumerate(nb):
        pad[i, :len(ix)] = ix
    P = P.astype(dtype)
    N = np.asarray(normals, np.float64).astype(dtype)
    I = intensity(colors, dtype)
    m = np.zeros((n, 6), dtype)
    atb = np.zeros((n, 3), dtype)
    for j in range(1, kmax):
        use = (cnt > j)[:, None]
        q = P[pad[:, j]]
        d = q - P
        dot = ((d[:, 0] * N[:, 0] + d[:, 1] * N[:, 1]) + d[:, 2] * N[:, 2])[:, None]
        a = np.where(use, (q - dot * N) - P, 0)
        b = np.where(use[:, 0], I[pad[:, j]] - I, 0)
        m += np.stack([a[:, 0] * a[:, 0], a[:, 0] * a[:, 1], a[:, 0] * a[:, 2], a[:, 1] * a[:, 1], a[:, 1] * a[:, 2], a[:, 2] * a[:, 2]], 1)
        atb += a * b[:, None]
    last = (cnt - 1).astype(dtype)[:, None] * N
    m += np.stack([last[:, 0] * last[:, 0], last[:, 0] * last[:, 1], last[:, 0] * last[:, 2], last[:, 1] * last[:, 1],
                   last[:, 1] * last[:, 2], last[:, 2] * last[:, 2]], 1)
    inv, det = _inv3_sym(m)
    with np.errstate(all="ignore"):
        g = np.stack([(inv[:, 0] * atb[:, 0] + inv[:, 1] * atb[:, 1]) + inv[:, 2] * atb[:, 2],
                      (inv[:, 1] * atb[:, 0] + inv[:, 3] * atb[:, 1]) + inv[:, 4] * atb[:, 2],
                      (inv[:, 2] * atb[:, 0] + inv[:, 4] * atb[:, 1]) + inv[:, 5] * atb[:, 2]], 1)
    ok = cnt >= 4
    if QUIRK_SINGULAR:
        ok &= np.isfinite(det) & (np.abs(det) >= 1e-300) & np.isfinite(g).all(1)
    g[~ok] = 0
    return I, g, cnt


def compute_transformation(s, t, nt, dt, it, i_s, lambda_geometric):
    """ComputeTransformation on correspondences: s current source points, t / nt / dt / it the matched target's position, normal,
    gradient and intensity, i_s the source intensities.  Returns the 4x4 update."""
    sg, sp = np.sqrt(lambda_geometric), np.sqrt(1.0 - lambda_geometric)
    e = ((s - t) * nt).sum(1)
    r_g = sg * e
    J_g = sg * np.concatenate([np.cross(s, nt), nt], 1)
    s1 = s - e[:, None] * nt
    i0 = (dt * (s1 - t)).sum(1) + it
    m = -(dt - (dt * nt).sum(1)[:, None] * nt)
    r_i = sp * (i_s - i0)
    J_i = sp * np.concatenate([np.cross(s, m), m], 1)
    JTJ = J_g.T @ J_g + J_i.T @ J_i
    JTr = J_g.T @ r_g + J_i.T @ r_i
    return co.solve_6x6(JTJ, JTr)[0]


def registration_colored(source, source_colors, target, target_normals, target_colors, max_dist, init=None,
                         lambda_geometric=LAMBDA_GEOMETRIC, max_iteration=30, relative_fitness=1e-6, relative_rmse=1e-6,
                         gradient_radius=None, gradient_max_nn=30, history=None):
    """registration_colored_icp: the generic RegistrationICP loop of co.registration around compute_transformation.
    Returns dict(T, fitness, inlier_rmse, iterations, correspondences)."""
    tgt = np.asarray(target, float)
    tn = np.asarray(target_normals, float)
    it, dt, _ = color_gradients(tgt, tn, target_colors, gradient_radius if gradient_radius else 2.0 * max_dist, gradient_max_nn)
    i_s = intensity(source_colors)
    T = np.eye(4) if init is None else np.array(init, float)
    P = co.transform_points(T, np.asarray(source, float))
    tree = cKDTree(tgt)
    i, j, fit, rmse = co._evaluate(P, tree, max_dist)
    k = 0
    for k in range(1, max_iteration + 1):
        U = np.eye(4) if i.size == 0 else compute_transformation(P[i], tgt[j], tn[j], dt[j], it[j], i_s[i], lambda_geometric)
        T = U @ T
        P = co.transform_points(U, P)
        pf, pr = fit, rmse
        i, j, fit, rmse = co._evaluate(P, tree, max_dist)
        if history is not None:
            history.append((fit, rmse))
        if abs(pf - fit) < relative_fitness and abs(pr - rmse) < relative_rmse:
            break
    return dict(T=T, fitness=fit, inlier_rmse=rmse, iterations=k, correspondences=int(i.size))


# ---- the test scene ("Coloured ICP"): a textured, nearly flat patch seen twice ----------------------------
def rigid_z(deg, t):
    a = np.radians(deg)
    T = np.eye(4)
    T[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
    T[:3, 3] = t
    return T


TRUE_MOTION = rigid_z(0.6, (0.006, -0.004, 0.001))


def field(x, y):
    return 0.5 + 0.25 * np.sin(40 * x) * np.cos(33 * y) + 0.15 * np.sin(17 * x + 23 * y)


def patch(n, rng, relief, noise):
    xy = rng.uniform(-0.25, 0.25, (n, 2))
    z = relief * np.sin(9 * xy[:, 0]) * np.cos(7 * xy[:, 1]) + rng.normal(0, noise, n)
    p = np.column_stack([xy, z])
    return p, field(xy[:, 0], xy[:, 1])


def colors_of(inten, tint=(1.0, 1.0, 1.0)):
    """colours whose mean is the intensity; a tint with mean 1 makes the three channels differ"""
    return inten[:, None] * np.asarray(tint, float)[None, :]


def scene(relief=0.0, noise=2e-4, nt=6000, ns=4000, seed=0, tint=(1.0, 1.0, 1.0)):
    """(source, source colours, target, target normals, target colours, true T): target and source points drawn independently
    on a 0.5 m x 0.5 m patch, z = relief sin(9x) cos(7y) + N(0, noise); the source is the patch moved by inv(TRUE_MOTION), so the
    registration should return TRUE_MOTION.  Target normals: the oracle's hybrid estimate (radius 0.04, 30 neighbours)."""
    rng = np.random.default_rng(seed)
    tgt, it = patch(nt, rng, relief, noise)
    src0, i_s = patch(ns, rng, relief, noise)
    src = co.transform_points(np.linalg.inv(TRUE_MOTION), src0)
    tn = co.estimate_normals_hybrid(tgt, 0.04, 30)
    return src, colors_of(i_s, tint), tgt, tn, colors_of(it, tint), TRUE_MOTION


def pose_error(T, T_true):
    """(translation error in metres, rotation error in degrees)"""
    D = np.asarray(T) @ np.linalg.inv(T_true)
    ang = np.degrees(np.arccos(np.clip((np.trace(D[:3, :3]) - 1) / 2, -1, 1)))
    return float(np.linalg.norm(np.asarray(T)[:3, 3] - T_true[:3, 3])), float(ang)
