"""The cases of tests/test_colored_step_ref.py (CPU: the conditions each case must meet) and tests/test_colored_step_gpu.py (the
coloured registration step on the device against tests/icp_step_ref.py, mode 3).  Deterministic, numpy only.  A case is a case of
tests/icp_step_cases.py (its geometry comes from there) with sc / tc (colours), lam (lambda_geometric), radius / nn (the gradient
search; 0: the call's defaults, twice the distance and 30), centre (what the colour field is laid around) and compare_step."""
import numpy as np

from tests import icp_step_cases as cs

TINT = (1.1, 1.0, 0.9)          # three distinct channels whose mean is the intensity field
LAMBDA = 0.968


def field(x, centre=(0.0, 0.0, 0.0)):
    """a smooth intensity in [0.1, 0.9] of the position relative to `centre`, with a period near the ellipsoid's size"""
    q = np.asarray(x, float) - np.asarray(centre, float)
    return 0.5 + 0.25 * np.sin(9 * q[:, 0] + 1) * np.cos(7 * q[:, 1]) + 0.15 * np.sin(5 * q[:, 1] + 8 * q[:, 2])


def tinted(inten):
    return inten[:, None] * np.asarray(TINT)[None, :]


def hashed(n):
    """[n,3] colours that are dyadic fractions k / 1024 in [0, 1) of a multiplicative hash of the row index: neighbouring rows
    have unrelated colours, the three channels differ, and (r + g) + b is exact"""
    k = np.arange(n, dtype=np.uint64)
    cols = [((k + np.uint64(1)) * np.uint64(m) % np.uint64(1 << 32)) >> np.uint64(22) for m in (2654435761, 2246822519, 3266489917)]
    return np.stack(cols, 1).astype(np.float64) / 1024.0


def colored(c, name=None, family=None, lam=LAMBDA, centre=(0.0, 0.0, 0.0), sc=None, tc=None, radius=0.0, nn=0, compare_step=True):
    """the coloured case of a case of icp_step_cases: the target's colours are the field at its points, the source's the field
    where the true motion takes them (about the field's centre)"""
    init = np.eye(4) if c["init"] is None else c["init"]
    at = cs.apply(cs.rigid((0.3, -0.5, 0.8), 1.0, (0.004, -0.003, 0.002), about=centre) @ init, c["src"])
    out = dict(c, name=name or c["name"], family=family or c["family"], lam=float(lam), centre=np.asarray(centre, float),
               radius=float(radius), nn=int(nn), compare_step=compare_step, modes=(3,),
               sc=np.ascontiguousarray(tinted(field(at, centre)) if sc is None else sc, dtype=np.float64),
               tc=np.ascontiguousarray(tinted(field(c["tgt"], centre)) if tc is None else tc, dtype=np.float64))
    return out


def chunk_cases():
    return [colored(c) for c in cs.chunk_cases()]


def large_case(cus):
    return colored(cs.large_case(cus))


def _base600():
    s, t, sn, tn = cs.sized(600)
    return cs._case("base600", "lambda", s, t, 0.05, sn=sn, tn=tn)


LAMBDAS = (0.0, 0.5, 0.968, 1.0)


def lambda_cases():
    return [colored(_base600(), name=f"lambda{lam:g}", lam=lam) for lam in LAMBDAS]


def permutation_cases():
    """the 600-source case in reversed and in a random order (the Morton sort of the set-up then moves every row), each with
    smooth colours and with hashed ones (a colour gathered from another row is then wrong by a large amount)"""
    b = _base600()
    orders = dict(reversed=np.arange(600)[::-1], shuffled=np.random.default_rng(5).permutation(600), given=np.arange(600))
    out = []
    for oname, order in orders.items():
        c = dict(b, src=np.ascontiguousarray(b["src"][order]), sn=np.ascontiguousarray(b["sn"][order]))
        if oname != "given":
            out.append(colored(c, name=f"{oname}_smooth", family="permutation"))
        out.append(colored(c, name=f"{oname}_hash", family="permutation", sc=hashed(600)))
    return out


MIXED_RADIUS = 0.06


def mixed_case():
    """the target: the x > 0 half of a 1600-point ellipsoid, and of its x < -0.07 part a subset whose points are further than
    0.065 from each other: within the gradient radius 0.06 a sparse point finds only itself, so its record is zero.  Half of
    the 600 sources are drawn from either part."""
    full, fn = cs.ellipsoid(1600, 31)
    dense = np.nonzero(full[:, 0] > 0)[0]
    keep = []
    for k in np.nonzero(full[:, 0] < -0.07)[0]:
        if all(np.linalg.norm(full[k] - full[q]) > 0.065 for q in keep):
            keep.append(k)
    sparse = np.array(keep)
    rng = np.random.default_rng(32)
    order = rng.permutation(len(dense) + len(sparse))                 # the two kinds interleaved in the caller's numbering
    idx = np.concatenate([dense, sparse])[order]
    is_sparse = (np.arange(len(idx)) >= len(dense))[order]
    tgt, tn = full[idx], fn[idx]
    pick = np.concatenate([rng.choice(np.nonzero(~is_sparse)[0], 300), rng.choice(np.nonzero(is_sparse)[0], 300)])
    Ti = np.linalg.inv(cs.MOTION)
    src = cs.apply(Ti, tgt[pick] + rng.normal(0, 2e-4, (600, 3)))
    c = colored(cs._case("mixed_gradients", "mixed", src, tgt, 0.05, sn=tn[pick] @ Ti[:3, :3].T, tn=tn), radius=MIXED_RADIUS)
    c["is_sparse"] = is_sparse
    return c


def masked_cases():
    return [colored(c) for c in cs.masked_cases()]


def init_case():
    """a 40 degree initial pose: J's p = T s differs from s by far more than a step"""
    tgt, tn = cs.ellipsoid(300, 21)
    init = cs.rigid((0.1, 0.7, -0.2), 40.0, (0.02, -0.01, 0.03))
    back = np.linalg.inv(cs.MOTION @ init)
    rng = np.random.default_rng(22)
    src = cs.apply(back, tgt + rng.normal(0, 2e-4, tgt.shape))
    return colored(cs._case("init40", "init", src, tgt, 0.05, init=init, sn=tn @ back[:3, :3].T, tn=tn))


STEP_COMPARED_UP_TO = 10.0      # the far offsets at which 32 err_x < 1e-6 (tests/test_colored_step_ref.py holds this)


def far_cases():
    return [colored(c, centre=off * np.array([1.0, -0.6, 0.8]), compare_step=off <= STEP_COMPARED_UP_TO)
            for c, off in zip(cs.far_cases(), cs.OFFSETS)]


def singular_case():
    """constant colours on the plane z = 0.25 with the normals (0, 0, 1): p x n = (p_y, -p_x, 0), so three columns of J are zero in
    every row, the gradients are zero, and det(J^T J) is exactly zero"""
    rng = np.random.default_rng(41)
    tgt = np.c_[(rng.random((300, 2)) - 0.5) * 0.6, np.full(300, 0.25)]
    src = tgt[rng.permutation(300)] + (0.002, 0.001, 0.003)
    tn = np.tile([[0.0, 0.0, 1.0]], (300, 1))
    c = cs._case("singular_plane", "singular", src, tgt, 0.05, sn=tn, tn=tn)
    return colored(c, sc=np.full((300, 3), 0.375), tc=np.full((300, 3), 0.375))


def scaled_normals_case():
    """target normals of lengths 0.6 to 1.4.  With unit normals every row of a gradient system lies in the tangent plane, so
    d . n = 0 to rounding and d . (p' - t) = d . (p - t): whether the predicted intensity is taken at p' = p - e n or at p
    cannot be seen.  Normals that are not unit vectors (nothing normalises them, as in the original) leave the gradient a
    component along n, and e (d . n) then stands far above the bound (tests/test_colored_step_ref.py measures by how much)."""
    b = _base600()
    length = np.random.default_rng(51).uniform(0.6, 1.4, len(b["tgt"]))
    return colored(dict(b, tn=np.ascontiguousarray(b["tn"] * length[:, None])), name="scaled_normals", family="normals")


def small_cases():
    return (chunk_cases() + lambda_cases() + permutation_cases() + [mixed_case()] + masked_cases() + [init_case()] + far_cases()
            + [singular_case(), scaled_normals_case()])


def gradient_setup(c):
    """(radius, max_nn) the call resolves for the case's target gradients"""
    return (c["radius"] if c["radius"] > 0 else 2.0 * c["md"]), (c["nn"] if c["nn"] > 0 else 30)
