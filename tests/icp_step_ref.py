"""Plain restatement of ONE step of the registration loop of csrc/cloud.hip (k_icp_eval -> icp_accumulate<MODE> -> k_icp_step ->
the point-to-point Umeyama step / solve6_to_matrix), for the modes 0 (point-to-point), 1 (point-to-plane), 2 (GICP) and
3 (coloured: r3d_debug_icp_sums_colored's slots, from the formulas of include/r3d.h).  numpy, no GPU.  Every sum and every 3x3 inverse is formed in np.longdouble; what the final factorisations take (LAPACK's SVD, det and
solve) is float64.

Correspondences come from tests/neighbor_ref.py: brute force under (squared distance, index) with a strict `<` against the
distance, on p = T * source formed with the kernels' own expression, so p and the squared distances equal the device's bit for bit.

Slot layout (include/r3d.h, r3d_debug_icp_sums): [0] count, [1] sum d2; point-to-point [2..4] sum q, [5..7] sum u,
[8 + 3a + b] sum q_a u_b with q = p - o, u = t - o; the other modes [2..22] the upper triangle of J^T J row by row and [23..28] J^T r.
Beside every slot stands the sum of the absolute values of its terms, a term being one elementary product of the data (the
products a Jacobian entry or a residual is made of are expanded, each taken by absolute value): the rounding bound of a float64
sum is stated against that figure.

Coloured mode: the target's records (intensity, gradient) and the source's intensities are INPUTS, like the normals; sg and sp are
the float64 square roots the host passes to the kernel.  Its expanded terms: e = d.n has the three d_a n_a (d = p - t, a datum
as in point-to-plane); m_a = -(g_a - (g.n) n_a) has g_a and the three g_b n_b n_a; the predicted intensity has, per axis,
g_a p_a, the three g_a d_b n_b n_a and g_a t_a (the kernel forms (p_a - e n_a) - t_a in that order, so p and t enter by their own
size, not by their difference), and I_t.  The longest chain of roundings behind one term of a slot: 8 in an entry of J_I
(3 in g.n, its product with n_a, the subtraction, the product with p, the cross product's subtraction, the scale sp), 14 in r_I, so
at most 8 + 14 + 1 = 23 in a product: the 64 of sum_bound covers the mode."""
import numpy as np

from tests import neighbor_ref as nr

LD = np.longdouble
P2P, P2PLANE, GICP, COLORED = 0, 1, 2, 3
NSLOTS = 29
U53 = 2.0 ** -53
TRIU = [(a, b) for a in range(6) for b in range(a, 6)]        # slot 2 + k  <->  JTJ[a][b]


def sum_bound(n_corr, abs_terms):
    """|float64 sum - exact| <= (n + 64) 2^-53 sum|terms|: n additions and up to 64 roundings inside a term"""
    return (n_corr + 64) * U53 * np.asarray(abs_terms, np.float64)


def effective_normals(normals):
    """Open3D's GetRotationFromE1ToX quirk: a normal with n_x < -0.99 (strictly) is replaced by e1"""
    n = np.array(normals, np.float64).reshape(-1, 3)
    n[n[:, 0] < -0.99] = (1.0, 0.0, 0.0)
    return n


def _inv3(M):
    """inverse of [n,3,3] matrices through the adjugate, in the dtype of M (np.linalg has no longdouble)"""
    c = np.empty_like(M)
    for i in range(3):
        for j in range(3):
            i1, i2, j1, j2 = (i + 1) % 3, (i + 2) % 3, (j + 1) % 3, (j + 2) % 3
            c[:, j, i] = M[:, i1, j1] * M[:, i2, j2] - M[:, i1, j2] * M[:, i2, j1]      # cofactor (i, j), transposed
    det = M[:, 0, 0] * c[:, 0, 0] + M[:, 0, 1] * c[:, 1, 0] + M[:, 0, 2] * c[:, 2, 0]
    return c / det[:, None, None]


def _skew_neg(p):
    """K = -[p]x for every row of p"""
    K = np.zeros((len(p), 3, 3), p.dtype)
    K[:, 0, 1], K[:, 0, 2] = p[:, 2], -p[:, 1]
    K[:, 1, 0], K[:, 1, 2] = -p[:, 2], p[:, 0]
    K[:, 2, 0], K[:, 2, 1] = p[:, 1], -p[:, 0]
    return K


def nearest(target, source, T, max_distance, threads=8):
    """neighbor_ref.brute_nearest; a large source goes through it in slices on a few threads (numpy releases the lock), every
    query is still compared with every target"""
    src = np.ascontiguousarray(source, np.float64).reshape(-1, 3)
    if len(src) < 20000:
        return nr.brute_nearest(target, src, T, max_distance)
    from concurrent.futures import ThreadPoolExecutor
    cuts = np.linspace(0, len(src), 4 * threads + 1).astype(int)
    with ThreadPoolExecutor(threads) as ex:
        parts = list(ex.map(lambda k: nr.brute_nearest(target, src[cuts[k]:cuts[k + 1]], T, max_distance), range(4 * threads)))
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def evaluate(source, target, max_distance, mode, T=None, source_normals=None, target_normals=None, gicp_epsilon=0.0, origin=None,
             pairs=None, colors=None):
    """One evaluation at pose T.  Returns a dict: n (count), i / j (the pairs), d2, value [29] and abs [29] (longdouble), p / t
    (the paired points, float64), cond_M (largest cond(M) of GICP, else 1), and for point-to-point mean_p, mean_t and sigma (the
    centred covariance (1/n) sum (t - mt)(p - mp)^T in longdouble) with sigma64, the same in float64.
    pairs: neighbor_ref.brute_nearest's result for these arguments, when the caller has it already (it depends on no mode).
    colors (mode 3): dict(src_intensity [ns], tgt_records [nt,4] (intensity, gradient), lambda_geometric).  The result then also
    has geometric / photometric: the (value, abs) slot vectors of either row alone, scale included (their sum is value / abs)."""
    T = np.eye(4) if T is None else np.asarray(T, np.float64).reshape(4, 4)
    src = np.ascontiguousarray(source, np.float64).reshape(-1, 3)
    tgt = np.ascontiguousarray(target, np.float64).reshape(-1, 3)
    corr, d2 = nearest(tgt, src, T, max_distance) if pairs is None else pairs
    i = np.nonzero(corr >= 0)[0]
    j = corr[i].astype(np.int64)
    n = len(i)
    p64, t64 = nr.transform(T, src)[i], tgt[j]
    p, t = p64.astype(LD), t64.astype(LD)
    val, ab = np.zeros(NSLOTS, LD), np.zeros(NSLOTS, LD)
    val[0] = ab[0] = n
    val[1] = ab[1] = d2[i].astype(LD).sum()
    out = dict(n=n, i=i, j=j, d2=d2[i], p=p64, t=t64, cond_M=1.0, value=val, abs=ab)
    if n == 0:
        return out
    if mode == P2P:
        o = np.zeros(3, LD) if origin is None else np.asarray(origin, np.float64).astype(LD)
        q, u = p - o, t - o
        val[2:5], ab[2:5] = q.sum(0), np.abs(q).sum(0)
        val[5:8], ab[5:8] = u.sum(0), np.abs(u).sum(0)
        for a in range(3):
            for b in range(3):
                val[8 + 3 * a + b] = (q[:, a] * u[:, b]).sum()
                ab[8 + 3 * a + b] = np.abs(q[:, a] * u[:, b]).sum()
        mp, mt = p.sum(0) / n, t.sum(0) / n
        out.update(mean_p=mp, mean_t=mt, sigma=(t - mt).T @ (p - mp) / n)
        mp64, mt64 = p64.mean(0), t64.mean(0)
        out["sigma64"] = (t64 - mt64).T @ (p64 - mp64) / n
        return out
    nt_ = np.asarray(target_normals, np.float64).reshape(-1, 3)[j]
    d = p - t
    if mode == P2PLANE:
        nn = nt_.astype(LD)
        J = np.concatenate([np.cross(p, nn), nn], 1)                                    # [n,6]
        pa, na = np.abs(p), np.abs(nn)
        Ja = np.concatenate([np.stack([pa[:, 1] * na[:, 2] + pa[:, 2] * na[:, 1], pa[:, 2] * na[:, 0] + pa[:, 0] * na[:, 2],
                                       pa[:, 0] * na[:, 1] + pa[:, 1] * na[:, 0]], 1), na], 1)
        r, ra = (d * nn).sum(1), (np.abs(d) * na).sum(1)
        JTJ, JTJa = J.T @ J, Ja.T @ Ja
        JTr, JTra = J.T @ r, Ja.T @ ra
    elif mode == COLORED:
        lam = float(colors["lambda_geometric"])
        sg, sp = LD(np.sqrt(lam)), LD(np.sqrt(1.0 - lam))
        rec = np.asarray(colors["tgt_records"], np.float64).reshape(-1, 4)[j].astype(LD)
        i_s, i_t, g = np.asarray(colors["src_intensity"], np.float64).reshape(-1)[i].astype(LD), rec[:, 0], rec[:, 1:]
        nn = nt_.astype(LD)
        pa, ta, na, ga, da = np.abs(p), np.abs(t), np.abs(nn), np.abs(g), np.abs(d)

        def cross_abs(x, y):
            return np.stack([x[:, 1] * y[:, 2] + x[:, 2] * y[:, 1], x[:, 2] * y[:, 0] + x[:, 0] * y[:, 2], x[:, 0] * y[:, 1] + x[:, 1] * y[:, 0]], 1)
        e, ea = (d * nn).sum(1), (da * na).sum(1)
        J_g, J_ga = sg * np.concatenate([np.cross(p, nn), nn], 1), sg * np.concatenate([cross_abs(pa, na), na], 1)
        r_g, r_ga = sg * e, sg * ea
        gn, gna = (g * nn).sum(1), (ga * na).sum(1)
        m, ma = -(g - gn[:, None] * nn), ga + gna[:, None] * na
        J_i, J_ia = sp * np.concatenate([np.cross(p, m), m], 1), sp * np.concatenate([cross_abs(pa, ma), ma], 1)
        i0 = (g * ((p - e[:, None] * nn) - t)).sum(1) + i_t
        i0a = (ga * (pa + ea[:, None] * na + ta)).sum(1) + np.abs(i_t)
        r_i, r_ia = sp * (i_s - i0), sp * (np.abs(i_s) + i0a)
        parts = []
        for Jx, rx, Jxa, rxa in ((J_g, r_g, J_ga, r_ga), (J_i, r_i, J_ia, r_ia)):
            pv, pab = np.zeros(NSLOTS, LD), np.zeros(NSLOTS, LD)
            A, Aa = Jx.T @ Jx, Jxa.T @ Jxa
            for k, (a, b) in enumerate(TRIU):
                pv[2 + k], pab[2 + k] = A[a, b], Aa[a, b]
            pv[23:29], pab[23:29] = Jx.T @ rx, Jxa.T @ rxa
            parts.append((pv, pab, A, Aa))
        out["geometric"], out["photometric"] = parts[0][:2], parts[1][:2]
        JTJ, JTJa = parts[0][2] + parts[1][2], parts[0][3] + parts[1][3]
        JTr, JTra = parts[0][0][23:29] + parts[1][0][23:29], parts[0][1][23:29] + parts[1][1][23:29]
    elif mode == GICP:
        eps = gicp_epsilon if gicp_epsilon > 0 else 1e-3
        a_ = effective_normals(nt_).astype(LD)
        s_ = effective_normals(np.asarray(source_normals, np.float64).reshape(-1, 3)[i]).astype(LD)
        R = T[:3, :3].astype(LD)
        b_ = s_ @ R.T
        w = LD(1.0) - LD(eps)
        eye = np.eye(3, dtype=LD)[None]
        M = 2 * eye - w * (a_[:, :, None] * a_[:, None, :] + b_[:, :, None] * b_[:, None, :])   # C_t + R C_s R^T
        out["cond_M"] = float(np.linalg.cond(M.astype(np.float64)).max())
        A = _inv3(M)
        Jb = np.concatenate([_skew_neg(p), np.broadcast_to(eye, (n, 3, 3))], 2)          # [n,3,6]
        Aa, Jba = np.abs(A), np.abs(Jb)
        JTJ = np.einsum("nri,nrj->ij", Jb, np.einsum("nrs,nsj->nrj", A, Jb))           # sum Jb^T A Jb
        JTJa = np.einsum("nri,nrj->ij", Jba, np.einsum("nrs,nsj->nrj", Aa, Jba))
        JTr = np.einsum("nri,nr->i", Jb, np.einsum("nrs,ns->nr", A, d))                # sum Jb^T A (p - t)
        JTra = np.einsum("nri,nr->i", Jba, np.einsum("nrs,ns->nr", Aa, np.abs(d)))
    else:
        raise ValueError(mode)
    for k, (a, b) in enumerate(TRIU):
        val[2 + k], ab[2 + k] = JTJ[a, b], JTJa[a, b]
    val[23:29], ab[23:29] = JTr, JTra
    out.update(JTJ=JTJ, JTr=JTr)
    return out


def p2p_from_slots(sums, origin):
    """(mean_p, mean_t, sigma) from a device's point-to-point slots by the header's formula"""
    s = np.asarray(sums, np.float64)
    n = s[0]
    mq, mu = s[2:5] / n, s[5:8] / n
    sigma = np.empty((3, 3))
    for a in range(3):
        for b in range(3):
            sigma[a, b] = s[8 + 3 * b + a] / n - mu[a] * mq[b]
    return np.asarray(origin, np.float64) + mq, np.asarray(origin, np.float64) + mu, sigma


def p2p_derived_bounds(ev):
    """Bounds on the means and on sigma derived from slots that each meet sum_bound (ev evaluated with the device's origin):
    first order in the slots' errors, plus two roundings of each division and product."""
    n = ev["n"]
    b = sum_bound(n, ev["abs"])
    v = np.abs(ev["value"].astype(np.float64))
    mq, mu = v[2:5] / n, v[5:8] / n
    bm_q, bm_u = b[2:5] / n + 2 * U53 * mq, b[5:8] / n + 2 * U53 * mu
    bs = np.empty((3, 3))
    for a in range(3):
        for c in range(3):
            k = 8 + 3 * c + a
            bs[a, c] = b[k] / n + mu[a] * bm_q[c] + mq[c] * bm_u[a] + 4 * U53 * (v[k] / n + mu[a] * mq[c])
    return bm_q, bm_u, bs


def euler_zyx(x):
    """TransformVector6dToMatrix4d: R = Rz(x2) Ry(x1) Rx(x0), t = x[3:]"""
    ca, sa, cb, sb, cc, sc = np.cos(x[0]), np.sin(x[0]), np.cos(x[1]), np.sin(x[1]), np.cos(x[2]), np.sin(x[2])
    U = np.eye(4)
    U[:3, :3] = [[cc * cb, cc * sb * sa - sc * ca, cc * sb * ca + sc * sa],
                 [sc * cb, sc * sb * sa + cc * ca, sc * sb * ca - cc * sa],
                 [-sb, cb * sa, cb * ca]]
    U[:3, 3] = x[3:]
    return U


def step(ev, mode):
    """The update U (4x4 float64) of one evaluation, and a dict of what bounds its float64 error.
    Point-to-point: centred moments -> SVD -> Eigen's Umeyama sign rule; info has sv (singular values), rank (singular values
    above 1e-6 of the largest), err_R = |sigma64 - sigma| / (sv[1] + sv[2]).  Other modes: the 6x6 solve with |det| < 1e-6 ->
    identity, then the ZYX Euler composition; info has det, solved, cond, err_x = cond 2^-53 |x|."""
    U = np.eye(4)
    if ev["n"] == 0:
        return U, dict(rank=0, solved=False, det=0.0, err_R=0.0, err_x=0.0)
    if mode == P2P:
        sigma = ev["sigma"].astype(np.float64)
        Us, sv, Vt = np.linalg.svd(sigma)
        S = np.ones(3)
        if np.linalg.det(Us) * np.linalg.det(Vt) < 0:
            S[2] = -1
        R = Us @ np.diag(S) @ Vt
        if sv[0] == 0:                                   # one pair, or coincident pairs: an SVD of the zero matrix is U = V = I
            R = np.eye(3)
        U[:3, :3] = R
        U[:3, 3] = (ev["mean_t"] - R.astype(LD) @ ev["mean_p"]).astype(np.float64)
        rank = int((sv > 1e-6 * max(sv[0], 1e-300)).sum()) if sv[0] > 0 else 0
        dsig = float(np.linalg.norm(ev["sigma64"] - sigma))
        den = sv[1] + sv[2]
        return U, dict(sv=sv, rank=rank, Us=Us, Vt=Vt, dsigma=dsig, err_R=dsig / den if den > 0 else (0.0 if sv[0] == 0 else np.inf))
    JTJ = np.zeros((6, 6))
    for k, (a, b) in enumerate(TRIU):
        JTJ[a, b] = JTJ[b, a] = float(ev["value"][2 + k])
    JTr = ev["value"][23:29].astype(np.float64)
    det = float(np.linalg.det(JTJ))
    if not np.isfinite(det) or abs(det) < 1e-6:
        return U, dict(det=det, solved=False, cond=np.inf, err_x=0.0)
    x = np.linalg.solve(JTJ, -JTr)
    cond = float(np.linalg.cond(JTJ))
    return euler_zyx(x), dict(det=det, solved=True, cond=cond, err_x=cond * U53 * float(np.linalg.norm(x)))


def step_tolerance(info, mode, T_expected):
    """What the device's U * init may differ by from the reference's: 32 x the reference's own float64 loss, with a floor of
    1e-14 (1 + |t|).  The 32 covers the other summation order and the Jacobi-vs-LAPACK route."""
    floor = 1e-14 * (1.0 + float(np.linalg.norm(np.asarray(T_expected)[:3, 3])))
    loss = info.get("err_R", 0.0) if mode == P2P else info.get("err_x", 0.0)
    return max(32.0 * loss, floor)


def rmse_tolerance(ev):
    """inlier_rmse = sqrt(S / n) with S within sum_bound of the reference's: the image of that interval, plus two roundings"""
    n = ev["n"]
    if n == 0:
        return 0.0
    S = float(ev["value"][1])
    B = float(sum_bound(n, ev["abs"][1]))
    return float(np.sqrt((S + B) / n) - np.sqrt(max(S - B, 0.0) / n)) + 4 * U53 * float(np.sqrt(S / n))


def rmse(ev):
    return float(np.sqrt(float(ev["value"][1]) / ev["n"])) if ev["n"] else 0.0
