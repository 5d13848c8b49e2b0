"""numpy restatement of the RGB-D odometry contract ("RGB-D odometry"), written from the contract and
not from the kernels.  [recalled, Open3D 0.18 pipelines/odometry/Odometry.cpp, RGBDOdometryJacobian.cpp, geometry/Image.cpp]:
Open3D is absent and the reference recorded no poses, so parity is UNPINNED; every choice memory leaves open is a named switch.

Planes are float32 [h][w]; poses are float64 4x4 mapping source camera coordinates to target camera coordinates; a camera
is the tuple (fx, fy, cx, cy)."""
import numpy as np

f32, f64 = np.float32, np.float64

# ---- named switches ---------------------------------------------------------------------------------------------------------
# u_t = (int)(p0 / z' + 0.5): the conversion truncates toward zero, so a projection in (-1.5, -0.5) lands in column 0.
# Off: floor(p0 / z' + 0.5), which drops those pixels.
QUIRK_TRUNCATING_ROUND = True
# Open3D rewrites both intensity planes in float32 (plane *= (float)scale).  The library keeps the planes and uses
# I = s * (double)plane wherever an intensity or an intensity gradient enters (at most one float32 rounding apart).  Off = the library.
QUIRK_NORMALIZE_IN_F32 = False
# the sums of an iteration taken in reversed list order: the restatement's own sensitivity to the summation order
SUMS_REVERSED = False

LAMBDA_DEPTH = 0.95
HYBRID, COLOR = 0, 1
DEFAULTS = dict(depth_diff_max=0.03, depth_min=0.0, depth_max=4.0, iterations=(20, 10, 5), levels=3)


def _seq_sum(terms):
    """float64 sum in list order (np.sum adds pairwise), along axis 0"""
    t = np.asarray(terms, dtype=f64)
    if SUMS_REVERSED:
        t = t[::-1]
    if t.shape[0] == 0:
        return np.zeros(t.shape[1:], f64)
    return np.cumsum(t, axis=0)[-1]


# ---- raw form: create_from_color_and_depth(convert_rgb_to_intensity=True) -------------------------------------------------
def convert_raw(color, depth, depth_scale=1000.0, depth_trunc=3.0, bgr=False):
    color = np.asarray(color, dtype=np.uint8)
    if color.ndim == 2 or color.shape[2] == 1:
        inten = color.reshape(color.shape[0], color.shape[1]).astype(f32) / f32(255.0)
    else:
        r, g, b = (color[..., 2 if bgr else 0].astype(f32), color[..., 1].astype(f32), color[..., 0 if bgr else 2].astype(f32))
        inten = ((f32(0.2990) * r + f32(0.5870) * g) + f32(0.1140) * b) / f32(255.0)
    z = np.asarray(depth, dtype=np.uint16).astype(f32) / f32(depth_scale)
    z = np.where(z > f32(depth_trunc), f32(0), z)       # the rule of r3d_backproject_depth, which the recorded PLY files pin
    return inten.astype(f32), z.astype(f32)


# ---- 3-tap passes: three taps added in float64 in tap order, rounded once to float32; replicated border ---------------------
def _pass(img, taps, axis):
    a = np.asarray(img, dtype=f32)
    pad = [(0, 0), (0, 0)]
    pad[axis] = (1, 1)
    p = np.pad(a, pad, mode="edge").astype(f64)
    n = a.shape[axis]
    sl = lambda o: tuple(slice(o, o + n) if ax == axis else slice(None) for ax in (0, 1))
    with np.errstate(invalid="ignore"):
        s = (f64(taps[0]) * p[sl(0)] + f64(taps[1]) * p[sl(1)]) + f64(taps[2]) * p[sl(2)]
    return s.astype(f32)


def gaussian3(img):
    return _pass(_pass(img, (0.25, 0.5, 0.25), 1), (0.25, 0.5, 0.25), 0)     # horizontal first, then vertical


def sobel3_dx(img):
    return _pass(_pass(img, (-1.0, 0.0, 1.0), 1), (1.0, 2.0, 1.0), 0)


def sobel3_dy(img):
    return _pass(_pass(img, (1.0, 2.0, 1.0), 1), (-1.0, 0.0, 1.0), 0)


def downsample(img):
    a = np.asarray(img, dtype=f32)
    h2, w2 = a.shape[0] // 2, a.shape[1] // 2
    p00, p01 = a[0:2 * h2:2, 0:2 * w2:2], a[0:2 * h2:2, 1:2 * w2:2]
    p10, p11 = a[1:2 * h2:2, 0:2 * w2:2], a[1:2 * h2:2, 1:2 * w2:2]
    with np.errstate(invalid="ignore"):
        return ((((p00 + p01) + p10) + p11) / f32(4.0)).astype(f32)


def prepare(intensity, depth, depth_min=0.0, depth_max=4.0, levels=3):
    """-> [(I_l, D_l)] for l = 0 .. levels-1 (un-normalised)"""
    d = np.asarray(depth, dtype=f32).copy()
    with np.errstate(invalid="ignore"):
        bad = (d > f32(depth_max)) | (d < f32(depth_min)) | (d <= 0) | np.isnan(d)
    d[bad] = np.nan
    out = [(gaussian3(np.asarray(intensity, dtype=f32)), gaussian3(d))]
    for _ in range(1, levels):
        i0, d0 = out[-1]
        out.append((downsample(gaussian3(i0)), downsample(d0)))
    return out


def gradients(i_l, d_l):
    """-> dI/dx, dI/dy, dD/dx, dD/dy (float32, not yet multiplied by 0.125; NaN depth gradients kept)"""
    return sobel3_dx(i_l), sobel3_dy(i_l), sobel3_dx(d_l), sobel3_dy(d_l)


def level_camera(cam, level):
    s = 0.5 ** level
    return tuple(f64(c) * s for c in cam)


def points(d_l, cam):
    """x = (u - cx) z / fx, y = (v - cy) z / fy, z in float64; [h][w][3]"""
    fx, fy, cx, cy = (f64(c) for c in cam)
    h, w = d_l.shape
    u, v = np.meshgrid(np.arange(w, dtype=f64), np.arange(h, dtype=f64))
    z = d_l.astype(f64)
    return np.stack([((u - cx) * z) / fx, ((v - cy) * z) / fy, z], -1)


def projection(T, cam):
    """M = K R K^-1 (row-major 9) and k = K t by explicit scalar expressions; with R = I the last row of M is exactly (0, 0, 1)"""
    fx, fy, cx, cy = (f64(c) for c in cam)
    T = np.asarray(T, dtype=f64)
    M = np.zeros(9, f64)
    A = [[fx * T[0, j] + cx * T[2, j] for j in range(3)], [fy * T[1, j] + cy * T[2, j] for j in range(3)], [T[2, j] for j in range(3)]]
    for i in range(3):
        M[i * 3 + 0] = A[i][0] / fx
        M[i * 3 + 1] = A[i][1] / fy
        M[i * 3 + 2] = (A[i][2] - (A[i][0] * cx) / fx) - (A[i][1] * cy) / fy
    k = np.array([fx * T[0, 3] + cx * T[2, 3], fy * T[1, 3] + cy * T[2, 3], T[2, 3]], f64)
    return M, k


def correspondences(d_src, d_tgt, T, cam, depth_diff_max=0.03, want_fragile=False):
    """-> int32 [n][4] rows (u_s, v_s, u_t, v_t) in target row-major order [, bool [h][w] of the target pixels a fragile
    source pixel reaches, number of fragile source pixels]"""
    h, w = d_src.shape
    M, k = projection(T, cam)
    u, v = np.meshgrid(np.arange(w, dtype=f64), np.arange(h, dtype=f64))
    d = d_src.astype(f64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        p = [d * ((M[i * 3] * u + M[i * 3 + 1] * v) + M[i * 3 + 2]) + k[i] for i in range(3)]
        zp = p[2]
        fu, fv = p[0] / zp + 0.5, p[1] / zp + 0.5
        live = ~np.isnan(d) & (zp > 0)
        if QUIRK_TRUNCATING_ROUND:
            inside = live & (fu > -1.0) & (fu < w) & (fv > -1.0) & (fv < h)
            conv = np.trunc
        else:
            inside = live & (fu >= 0.0) & (fu < w) & (fv >= 0.0) & (fv < h)
            conv = np.floor
        ut = np.where(inside, conv(np.where(inside, fu, 0.0)), 0).astype(np.int64)
        vt = np.where(inside, conv(np.where(inside, fv, 0.0)), 0).astype(np.int64)
        dt = d_tgt.astype(f64)[vt, ut]
        diff = np.abs(zp - dt)
        keep = inside & ~np.isnan(dt) & (diff <= f64(depth_diff_max))
    src_idx = (v * w + u).astype(np.int64)
    ks, kt = src_idx[keep], (vt * w + ut)[keep]
    zf = zp[keep].astype(f32)                              # the float32 narrowing of z' is part of the contract
    key = (zf.view(np.uint32).astype(np.uint64) << np.uint64(32)) | ks.astype(np.uint64)
    order = np.lexsort((key, kt))                          # by target pixel, then by (z', source index)
    kt_s, ks_s, key_s = kt[order], ks[order], key[order]
    first = np.ones(len(kt_s), bool)
    first[1:] = kt_s[1:] != kt_s[:-1]
    wt, ws = kt_s[first], ks_s[first]
    corr = np.stack([ws % w, ws // w, wt % w, wt // w], -1).astype(np.int32).reshape(-1, 4)
    if not want_fragile:
        return corr
    eps = 1e-9
    with np.errstate(invalid="ignore"):
        near = lambda f: np.abs(f - np.rint(f)) < eps
        frag = live & (near(fu) | near(fv))
        frag |= inside & ~np.isnan(dt) & (np.abs(diff - f64(depth_diff_max)) < eps)
    # a collision decided by less than one float32 step: winner and runner-up differ in double but not by a float32 step
    second = np.zeros(len(kt_s), bool)
    second[1:] = ~first[1:] & first[:-1]
    z_sorted = zp[keep][order]
    zi = np.nonzero(second)[0]
    if len(zi):
        za, zb = z_sorted[zi - 1], z_sorted[zi]
        close = (za != zb) & (np.abs(za - zb) <= np.spacing(np.maximum(za, zb).astype(f32)).astype(f64))
        fl = frag.reshape(-1)
        fl[ks_s[zi[close]]] = True
        fl[ks_s[zi[close] - 1]] = True
        frag = fl.reshape(h, w)
    reach = np.zeros((h, w), bool)
    fy_, fx_ = np.nonzero(frag)
    for du in (-eps, eps):
        for dv in (-eps, eps):
            a, b = np.trunc(fu[fy_, fx_] + du), np.trunc(fv[fy_, fx_] + dv)
            ok = (a >= 0) & (a < w) & (b >= 0) & (b < h)
            reach[b[ok].astype(int), a[ok].astype(int)] = True
    return corr, reach, int(frag.sum())


def normalisation(i_src, i_tgt, corr):
    """-> s_src, s_tgt (0.5 / mean over the list), or None for an empty list"""
    if len(corr) == 0:
        return None
    n = f64(len(corr))
    ms = _seq_sum(i_src[corr[:, 1], corr[:, 0]].astype(f64)) / n
    mt = _seq_sum(i_tgt[corr[:, 3], corr[:, 2]].astype(f64)) / n
    return f64(0.5) / ms, f64(0.5) / mt


def _scaled(plane, s):
    if QUIRK_NORMALIZE_IN_F32:
        return (plane.astype(f32) * f32(s)).astype(f64)
    return f64(s) * plane.astype(f64)


def iteration_sums(corr, pts_src, i_src, i_tgt, d_tgt, grads, T, cam, s_src, s_tgt, jacobian=HYBRID):
    """-> 29 numbers in solve6_to_matrix's slots (count, sum r^2, the upper triangle of JTJ row by row, JTr) and the same
    slots filled with the sums of |term|"""
    fx, fy = f64(cam[0]), f64(cam[1])
    T = np.asarray(T, dtype=f64)
    us, vs, ut, vt = (corr[:, i] for i in range(4))
    P = pts_src[vs, us]
    x = ((T[0, 0] * P[:, 0] + T[0, 1] * P[:, 1]) + T[0, 2] * P[:, 2]) + T[0, 3]
    y = ((T[1, 0] * P[:, 0] + T[1, 1] * P[:, 1]) + T[1, 2] * P[:, 2]) + T[1, 3]
    z = ((T[2, 0] * P[:, 0] + T[2, 1] * P[:, 1]) + T[2, 2] * P[:, 2]) + T[2, 3]
    gix, giy, gdx, gdy = grads
    if jacobian == HYBRID:
        a, b = np.sqrt(f64(1.0) - f64(LAMBDA_DEPTH)), np.sqrt(f64(LAMBDA_DEPTH))
    else:
        a, b = f64(1.0), f64(0.0)
    It, Is = _scaled(i_tgt[vt, ut], s_tgt), _scaled(i_src[vs, us], s_src)
    r0 = a * (It - Is)
    gx, gy = 0.125 * _scaled(gix[vt, ut], s_tgt), 0.125 * _scaled(giy[vt, ut], s_tgt)
    c0, c1 = (gx * fx) / z, (gy * fy) / z
    c2 = -(c0 * x + c1 * y) / z
    J0 = [a * (-z * c1 + y * c2), a * (z * c0 - x * c2), a * (-y * c0 + x * c1), a * c0, a * c1, a * c2]
    rows, res = [J0], [r0]
    if jacobian == HYBRID:
        qx, qy = gdx[vt, ut].astype(f64), gdy[vt, ut].astype(f64)
        qx, qy = 0.125 * np.where(np.isnan(qx), 0.0, qx), 0.125 * np.where(np.isnan(qy), 0.0, qy)
        r1 = b * (d_tgt[vt, ut].astype(f64) - z)
        d0, d1 = (qx * fx) / z, (qy * fy) / z
        d2 = -(d0 * x + d1 * y) / z
        J1 = [b * ((-z * d1 + y * d2) - y), b * ((z * d0 - x * d2) + x), b * (-y * d0 + x * d1), b * d0, b * d1, b * (d2 - 1.0)]
        rows.append(J1)
        res.append(r1)
    n = len(corr)
    terms, q = np.zeros((n, 29), f64), 2
    mags = np.zeros((n, 29), f64)
    terms[:, 0] = mags[:, 0] = 1.0

    def put(slot, parts):
        acc, mag = parts[0], np.abs(parts[0])
        for t in parts[1:]:
            acc, mag = acc + t, mag + np.abs(t)
        terms[:, slot], mags[:, slot] = acc, mag

    put(1, [r * r for r in res])
    for i in range(6):
        for j in range(i, 6):
            put(q, [J[i] * J[j] for J in rows])
            q += 1
    for i in range(6):
        put(23 + i, [J[i] * r for J, r in zip(rows, res)])
    return _seq_sum(terms), _seq_sum(mags)


def solve6_to_matrix(s, det_tol=1e-6):
    """x = LDLT(JTJ) \\ (-JTr), failure when |det| < det_tol; R = Rz(x2) Ry(x1) Rx(x0).  -> (ok, U)"""
    A = np.zeros((6, 6), f64)
    q = 2
    for a in range(6):
        for c in range(a, 6):
            A[a, c] = A[c, a] = s[q]
            q += 1
    b = -np.asarray(s[23:29], dtype=f64)
    L, Dg, det = np.zeros((6, 6), f64), np.zeros(6, f64), f64(1.0)
    with np.errstate(all="ignore"):
        for j in range(6):
            d = A[j, j]
            for k in range(j):
                d = d - L[j, k] * L[j, k] * Dg[k]
            Dg[j] = d
            det = det * d
            L[j, j] = 1.0
            for i in range(j + 1, 6):
                v = A[i, j]
                for k in range(j):
                    v = v - L[i, k] * L[j, k] * Dg[k]
                L[i, j] = v / d if d != 0 else 0.0
        U = np.eye(4)
        if not np.isfinite(det) or abs(det) < det_tol:
            return False, U
        y, x = np.zeros(6, f64), np.zeros(6, f64)
        for i in range(6):
            y[i] = b[i]
            for k in range(i):
                y[i] = y[i] - L[i, k] * y[k]
        y = y / Dg
        for i in range(5, -1, -1):
            x[i] = y[i]
            for k in range(i + 1, 6):
                x[i] = x[i] - L[k, i] * x[k]
    ca, sa, cb, sb, cc, sc = np.cos(x[0]), np.sin(x[0]), np.cos(x[1]), np.sin(x[1]), np.cos(x[2]), np.sin(x[2])
    U[:3, :3] = [[cc * cb, cc * sb * sa - sc * ca, cc * sb * ca + sc * sa], [sc * cb, sc * sb * sa + cc * ca, sc * sb * ca - cc * sa],
                 [-sb, cb * sa, cb * ca]]
    U[:3, 3] = x[3:]
    return True, U


def information(d_src, d_tgt, T, cam, depth_diff_max=0.03):
    """-> 6x6 matrix, its sums of |term|, number of correspondences (level 0, at T)"""
    corr = correspondences(d_src, d_tgt, T, cam, depth_diff_max)
    P = points(d_tgt, cam)[corr[:, 3], corr[:, 2]]
    x, y, z = P[:, 0], P[:, 1], P[:, 2]
    o, l, n = np.ones_like(x), np.zeros_like(x), len(corr)
    rows = [[l, z, -y, o, l, l], [-z, l, x, l, o, l], [y, -x, l, l, l, o]]
    G, Gm = np.zeros((6, 6)), np.zeros((6, 6))
    for i in range(6):
        for j in range(i, 6):
            t = (rows[0][i] * rows[0][j] + rows[1][i] * rows[1][j]) + rows[2][i] * rows[2][j]
            m = (np.abs(rows[0][i] * rows[0][j]) + np.abs(rows[1][i] * rows[1][j])) + np.abs(rows[2][i] * rows[2][j])
            G[i, j] = G[j, i] = _seq_sum(t)
            Gm[i, j] = Gm[j, i] = _seq_sum(m)
    return G, Gm, n


class Prepared:
    """both pyramids, the target gradients and source points per level, and the scales at odo_init"""

    def __init__(self, src, tgt, cam, init=None, depth_diff_max=0.03, depth_min=0.0, depth_max=4.0, levels=3, **_):
        self.cam, self.levels, self.depth_diff_max = tuple(f64(c) for c in cam), levels, depth_diff_max
        self.src = prepare(src[0], src[1], depth_min, depth_max, levels)
        self.tgt = prepare(tgt[0], tgt[1], depth_min, depth_max, levels)
        self.cams = [level_camera(self.cam, l) for l in range(levels)]
        self.grads = [gradients(*self.tgt[l]) for l in range(levels)]
        self.pts = [points(self.src[l][1], self.cams[l]) for l in range(levels)]
        self.init = np.eye(4) if init is None else np.asarray(init, dtype=f64).reshape(4, 4)
        self.corr_init = correspondences(self.src[0][1], self.tgt[0][1], self.init, self.cams[0], depth_diff_max)
        self.scales = normalisation(self.src[0][0], self.tgt[0][0], self.corr_init)

    def corr(self, level, T, want_fragile=False):
        return correspondences(self.src[level][1], self.tgt[level][1], T, self.cams[level], self.depth_diff_max, want_fragile)

    def sums(self, level, T, corr, jacobian=HYBRID):
        return iteration_sums(corr, self.pts[level], self.src[level][0], self.tgt[level][0], self.tgt[level][1], self.grads[level],
                              T, self.cams[level], self.scales[0], self.scales[1], jacobian)

    def step(self, level, T, jacobian=HYBRID):
        """-> corr, sums, |sums|, ok, pose after the step"""
        corr = self.corr(level, T)
        s, m = self.sums(level, T, corr, jacobian)
        ok, U = (False, np.eye(4)) if len(corr) == 0 else solve6_to_matrix(s)
        return corr, s, m, ok, U @ np.asarray(T, dtype=f64)


def compute_rgbd_odometry(src, tgt, cam, init=None, jacobian=HYBRID, **option):
    """src, tgt: (intensity, depth) float32 planes.  -> dict(success, T, info, info_mag, trace, failed_level, failed_iteration,
    correspondences_init, correspondences, r2)"""
    opt = dict(DEFAULTS, **option)
    levels, iters = opt["levels"], list(opt["iterations"]) + [0] * 4
    pr = Prepared(src, tgt, cam, init, **opt)
    fail = dict(success=0, T=np.eye(4), info=np.eye(6), info_mag=np.zeros((6, 6)), trace=[], correspondences_init=len(pr.corr_init),
                correspondences=0, r2=0.0)
    if pr.scales is None:
        return dict(fail, failed_level=0, failed_iteration=-1)
    T, trace, r2 = pr.init.copy(), [], 0.0
    for n_lv, level in enumerate(range(levels - 1, -1, -1)):
        for it in range(iters[n_lv]):
            _, s, _, ok, T = pr.step(level, T, jacobian)
            if not ok:
                return dict(fail, trace=trace, failed_level=level, failed_iteration=it)
            r2 = s[1]
            trace.append(T.copy())
    G, Gm, n = information(pr.src[0][1], pr.tgt[0][1], T, pr.cams[0], opt["depth_diff_max"])
    return dict(success=1, T=T, info=G, info_mag=Gm, trace=trace, failed_level=-1, failed_iteration=-1,
                correspondences_init=len(pr.corr_init), correspondences=n, r2=r2)


def pose_error(T, truth):
    return float(np.abs(np.asarray(T) - np.asarray(truth)).max())
