"""The cases of tests/test_icp_step_ref.py (CPU: the conditions each case must meet) and tests/test_icp_step_gpu.py (the device
against tests/icp_step_ref.py).  Deterministic, numpy only.  A case is a dict: name, family, src, tgt, md (max distance), init,
sn / tn (normals), eps (gicp_epsilon), modes."""
import numpy as np

ICP_BLOCK = 256
ALL = (0, 1, 2)


def rigid(axis, deg, t, about=(0.0, 0.0, 0.0)):
    """rotation by deg about the axis through the point `about`, then the translation t"""
    a = np.asarray(axis, float) / np.linalg.norm(axis)
    th = np.radians(deg)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    R = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)
    T = np.eye(4)
    T[:3, :3] = R
    c = np.asarray(about, float)
    T[:3, 3] = c - R @ c + np.asarray(t, float)
    return T


def apply(T, p):
    return p @ T[:3, :3].T + T[:3, 3]


SCALE = np.array([1.0, 0.7, 0.5])


def ellipsoid(n, seed, radius=0.3, noise=2e-4, centre=(0.0, 0.0, 0.0)):
    """(points, outward unit normals) of a noisy ellipsoid with half-axes radius * (1, 0.7, 0.5)"""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    p = v * SCALE * radius
    nrm = v / SCALE
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    return p + rng.normal(0, noise, (n, 3)) + np.asarray(centre, float), nrm


def _unit(rng, n):
    v = rng.standard_normal((n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _case(name, family, src, tgt, md, modes=ALL, init=None, sn=None, tn=None, eps=1e-3):
    src, tgt = np.ascontiguousarray(src, np.float64), np.ascontiguousarray(tgt, np.float64)
    rng = np.random.default_rng(len(src) * 7919 + len(tgt))
    return dict(name=name, family=family, src=src, tgt=tgt, md=float(md), modes=tuple(modes), init=init,
                sn=_unit(rng, len(src)) if sn is None else np.ascontiguousarray(sn, np.float64),
                tn=_unit(rng, len(tgt)) if tn is None else np.ascontiguousarray(tn, np.float64), eps=float(eps))


MOTION = rigid((0.3, -0.5, 0.8), 1.0, (0.004, -0.003, 0.002))


def sized(ns, nt=500, seed=0):
    """ns sources drawn from an nt-point ellipsoid (with repeats when ns > nt), moved by the inverse of a small motion"""
    tgt, tn = ellipsoid(nt, 100 + seed)
    rng = np.random.default_rng(ns)
    pick = rng.integers(0, nt, ns)
    Ti = np.linalg.inv(MOTION)
    src = apply(Ti, tgt[pick] + rng.normal(0, 2e-4, (ns, 3)))
    return src, tgt, tn[pick] @ Ti[:3, :3].T, tn


def chunk_cases():
    out = []
    for ns in (1, 63, 64, 65, 255, 256, 257):
        s, t, sn, tn = sized(ns)
        out.append(_case(f"ns{ns}", "chunks", s, t, 0.05, sn=sn, tn=tn))
    for chunks, ns in ((8, 2043), (16, 4000), (24, 6100), (9, 2200), (13, 3300)):
        assert (ns + ICP_BLOCK - 1) // ICP_BLOCK == chunks
        s, t, sn, tn = sized(ns)
        out.append(_case(f"chunks{chunks}", "chunks", s, t, 0.05, sn=sn, tn=tn))
    return out


def large_case(cus):
    """more chunks than workgroups (3 per CU) and a remainder, under the XCD split"""
    ns = (3 * cus + 1) * ICP_BLOCK + 17
    s, t, sn, tn = sized(ns, 2000)
    return _case(f"large_cus{cus}", "chunks", s, t, 0.05, sn=sn, tn=tn)


def masked_cases():
    s, t, sn, tn = sized(600)
    half = s.copy()
    half[::2] += (0.0, 0.0, 5.0)                                  # every other source far above the target
    lead = np.concatenate([s[:300], s + (-5.0, -5.0, -5.0)])      # 600 sources in one far cell: a run holding whole chunks
    none = s + (3.0, 0.0, 0.0)
    return [_case("half_far", "masked", half, t, 0.05, sn=sn, tn=tn),
            _case("chunk_of_zeros", "masked", lead, t, 0.05, sn=np.concatenate([sn[:300], sn]), tn=tn),
            _case("no_correspondence", "masked", none, t, 0.05, sn=sn, tn=tn)]


def boundary_cases():
    tgt = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0.5]], float)
    out = []
    for name, x in (("at_distance", 0.25), ("one_ulp_inside", np.nextafter(0.25, 0.0))):
        src = np.array([[x, 0, 0], [1.0625, 0, 0], [0, 1.125, 0], [0, 0, 0.875], [1, 1, 0.53125]], float)
        out.append(_case(name, "boundary", src, tgt, 0.25))
    return out


def few_pair_cases():
    rng = np.random.default_rng(42)
    T = rigid((0.2, 0.9, -0.4), 1.0, (0.003, 0.002, -0.004))
    Ti = np.linalg.inv(T)
    out = []
    for k in (1, 2, 3, 4, 5):
        tgt = (rng.random((k, 3)) - 0.5) * 0.6 + (0.1, 0.2, 1.0)
        out.append(_case(f"pairs{k}", "few", apply(Ti, tgt), tgt, 0.05))
    line = np.array([0.1, 0.2, 1.0]) + np.linspace(-0.3, 0.3, 6)[:, None] * np.array([0.6, -0.3, 0.74])
    out.append(_case("collinear6", "few", apply(Ti, line), line, 0.05))
    tgt, _ = ellipsoid(300, 7)
    tn = np.tile([[0.6, 0.0, 0.8]], (300, 1))
    out.append(_case("parallel_normals", "few", apply(Ti, tgt), tgt, 0.05, modes=(1, 2), tn=tn))
    return out


THICKNESS = (0.0, 1e-9, 1e-6, 1e-4, 1e-2)


def flat_cases():
    """a tilted plane patch of extent 0.6 at depth 1.5, 300 points, with a thickness normal to the plane"""
    out = []
    tilt = rigid((1.0, 0.4, 0.0), 25.0, (0, 0, 0))[:3, :3]
    for th in THICKNESS:
        for seed in (0, 1, 2):
            for deg in (1.0, 5.0):
                rng = np.random.default_rng(1000 + seed)
                local = np.c_[(rng.random((300, 2)) - 0.5) * 0.6, th * rng.standard_normal(300)]
                tgt = local @ tilt.T + (0.05, -0.1, 1.5)
                T = rigid((0.5, -0.3, 0.7), deg, (0.003, -0.002, 0.004), about=(0.05, -0.1, 1.5))
                src = apply(np.linalg.inv(T), tgt)[rng.permutation(300)]
                out.append(_case(f"flat_th{th:g}_s{seed}_{deg:g}deg", "flat", src, tgt, 0.1, modes=(0,)))
    return out


OFFSETS = (0.0, 10.0, 100.0, 1000.0)


def far_cases():
    out = []
    for c in OFFSETS:
        centre = c * np.array([1.0, -0.6, 0.8])
        tgt, tn = ellipsoid(1000, 11, centre=centre)
        T = rigid((0.3, -0.5, 0.8), 1.0, (0.004, -0.003, 0.002), about=centre)
        Ti = np.linalg.inv(T)
        rng = np.random.default_rng(12)
        src = apply(Ti, tgt + rng.normal(0, 2e-4, tgt.shape))
        out.append(_case(f"far_c{c:g}", "far", src, tgt, 0.05, sn=tn @ Ti[:3, :3].T, tn=tn))
    return out


QUIRK_NX = (-1.0, -0.995, -0.99, -0.985)


def gicp_cases():
    """normals either side of the n_x < -0.99 rule on both clouds, a few zero normals (M = 2 I), every epsilon, and a 40 degree
    initial pose so that R C_s R^T differs from C_s"""
    out = []
    for eps, deg in ((0.0, 0.0), (1e-3, 0.0), (0.5, 0.0), (1.0, 0.0), (1e-3, 40.0)):
        tgt, tn = ellipsoid(300, 21)
        init = rigid((0.1, 0.7, -0.2), deg, (0.02, -0.01, 0.03)) if deg else None
        back = np.linalg.inv(MOTION @ init) if deg else np.linalg.inv(MOTION)
        rng = np.random.default_rng(22)
        src = apply(back, tgt + rng.normal(0, 2e-4, tgt.shape))             # source k pairs with target k
        sn = tn @ back[:3, :3].T
        tn, sn = tn.copy(), sn.copy()
        for k, nx in enumerate(QUIRK_NX):
            q = (nx, np.sqrt(max(1.0 - nx * nx, 0.0)), 0.0)
            tn[10 + k], sn[20 + k] = q, q
            tn[30 + k], sn[30 + k] = q, q
        tn[0:3], sn[0:3], tn[40:42], sn[50:52] = 0.0, 0.0, 0.0, 0.0
        out.append(_case(f"gicp_eps{eps:g}_init{deg:g}", "gicp", src, tgt, 0.05, modes=(2,), init=init, sn=sn, tn=tn, eps=eps))
    return out


def small_cases():
    return chunk_cases() + masked_cases() + boundary_cases() + few_pair_cases() + flat_cases() + far_cases() + gicp_cases()
