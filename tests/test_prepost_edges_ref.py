"""CPU checks of the pre/post edge cases (tests/prepost_cases.py): every WLS case must give the filter real work, so that
the GPU tests built on them cannot pass on a trivial output, and the allowance for the partitioned solver must stay narrow
enough that it cannot excuse a real difference.  Also pins the float64 restatement of the smoother to the float32 one."""
import numpy as np
import pytest

from oracle import prepost_oracle as po
from tests import prepost_cases as pc

ALL = [(t, c) for t, cases in pc.TABLES.items() for c in cases]
IDS = [f"{t}-{c.id}" for t, c in ALL]


def test_every_case_of_the_issue_is_in_the_tables():
    solved = {1, 2, 31, 32, 33, 63, 64, 65, 95, 96, 97, 255, 256, 257, 288, 289, 512, 544, 545}
    shapes = {(c.W, c.H) for c in pc.SOLVER}
    assert {(n, 3) for n in solved} | {(3, n) for n in solved} <= shapes
    assert {(33, 63), (33, 64), (33, 65), (63, 33), (64, 33), (65, 33), (64, 65), (97, 64)} <= shapes
    assert {n // 32 for n in solved} >= {0, 1, 8, 9, 16, 17}                       # separators per line
    assert all((c.lam, c.sigma, c.radius, c.num_iter) == (8000.0, 1.5, 3, 3) for c in pc.SOLVER)
    assert all((c.W, c.H) == (97, 64) for c in pc.PARAMS)
    assert {c.num_iter for c in pc.PARAMS} >= {1, 2, 5, 16} and {c.lam for c in pc.PARAMS} >= {0.0, 500.0, 64000.0}
    assert {c.att for c in pc.PARAMS} >= {1.0} and {c.sigma for c in pc.PARAMS} >= {0.5, 25.0}
    assert {(c.guide_cn, c.guide_pad) for c in pc.PARAMS} >= {(3, 5), (1, 3)} and {c.lrc for c in pc.PARAMS} >= {1, 1000}
    dd = {(c.W, c.H, c.radius) for c in pc.DD}
    assert {(w, h, r) for w, h in ((65, 33), (130, 31)) for r in (0, 1, 2, 3, 4, 5, 6, 7, 12, 32)} <= dd
    assert {(w, h, r) for r in (6, 32) for w, h in ((1, 1), (2, 3), (3, 2), (5, 40), (40, 5))} <= dd
    assert {(70, h, 5) for h in (31, 32, 33, 64, 65)} <= dd
    assert [(c.min_disp, c.num_disp) for c in pc.ROI] == [(0, 16), (-8, 16), (3, 16), (-20, 16), (0, 80), (-100, 16)]
    assert [c.roi()[1] for c in pc.ROI] == [64, 64, 61, 60, 0, 0] and all((c.W, c.H) == (80, 20) for c in pc.ROI)


@pytest.mark.parametrize("table,c", ALL, ids=IDS)
def test_wls_case_gives_the_filter_work(table, c):
    r = pc.reference(c)
    lx, lw = c.roi()
    assert r.q32.shape == r.q64.shape == (c.H, lw) and r.want.dtype == np.int16 and r.conf.dtype == np.float32
    assert (r.want[:, :lx] == 16 * (c.min_disp - 1)).all() and (r.want[:, lx + lw:] == 16 * (c.min_disp - 1)).all()
    assert not r.conf[:, :lx].any() and not r.conf[:, lx + lw:].any()
    if lw * c.H < pc.MIN_PIXELS or c.lam <= 0:
        return
    conf = r.conf[:, lx:lx + lw]
    assert (conf > 0).mean() >= 0.80
    if c.radius > 0:                       # radius 0: the box variance of one pixel is 0, the confidence is 0 or 255 by construction
        assert ((conf > 0) & (conf < 255)).mean() >= 0.30
    assert (conf == 0).mean() >= 0.01
    assert (r.want[:, lx:lx + lw] != r.dl[:, lx:lx + lw]).mean() >= 0.25
    assert r.ambiguous.mean() <= 0.01      # the band that may excuse a one-LSB difference stays a small part of the case
    assert 0 < r.e < 1e-3


def test_lr_branches_are_all_taken():
    """The generator drives each branch of the LR-consistency test: partner outside the right ROI, agreeing, disagreeing."""
    c = pc.ROI[3]                                                # minD + D < 0: right ROI starts at x = 20
    dl, dr, _ = pc.case_inputs(c)
    (lx, _, lw, _), (rx, _, rw, _) = po.wls_rois(c.W, c.H, c.min_disp, c.num_disp)
    j = np.arange(c.W)[None, :].repeat(c.H, 0)[:, lx:lx + lw]
    ridx = j - (dl[:, lx:lx + lw].astype(int) >> 4)
    inside = (ridx >= rx) & (ridx < rx + rw)
    agree = np.abs(dl[:, lx:lx + lw].astype(int) + dr[np.arange(c.H)[:, None], np.clip(ridx, 0, c.W - 1)]) < c.lrc
    assert (~inside).mean() > 0.02 and (inside & agree).mean() > 0.5 and (inside & ~agree).mean() > 0.02
    assert (dl == -16).any() and (dl >> 4).max() >= 3


def test_uniform_random_disparities_would_test_nothing():
    """Why the generator is not rng.integers: the box variance of noise over a 64 px disparity range (x16) is far above
    1 / roll_off and puts the confidence to 0 everywhere."""
    rng = np.random.default_rng(0)
    dl = rng.integers(0, 1024, (20, 80)).astype(np.int16)
    dr = (-rng.integers(0, 1024, (20, 80))).astype(np.int16)
    assert not po.wls_confidence(dl, dr, 0, 0, 3).any()


@pytest.mark.parametrize("c", [pc.SOLVER[8], pc.PARAMS[3], pc.PARAMS[10], pc.ROI[1]], ids=lambda c: c.id)
def test_float64_smoother_restates_the_float32_one(c):
    """fgs_filter64 solves the systems fgs_filter solves: one pass leaves a float64-sized residual in (I + lam * L) u = f, and
    the whole filter lies within the forward error bound of a float32 solve of the float32 result."""
    r = pc.reference(c)
    lx, lw = c.roi()
    g = r.guide[:, lx:lx + lw]
    ch, cv = po.fgs_weights(g, po.fgs_lut(c.sigma, c.guide_cn))
    src = r.conf[:, lx:lx + lw]
    a32 = po.fgs_filter(src, ch, cv, c.lam, c.att, c.num_iter)
    a64 = po.fgs_filter64(src, ch, cv, c.lam, c.att, c.num_iter)
    assert a64.dtype == np.float64 and a32.dtype == np.float32
    # forward error of a float32 solve: condition number of I + lam * L (<= 1 + 4 lam, weights in [0, 1]) times the unit roundoff
    assert np.abs(a32 - a64).max() <= (1 + 4 * float(c.lam)) * 2.0 ** -23 * max(1.0, np.abs(a64).max())
    # the solved system: (I + lam * L) u = f for one horizontal pass, residual in float64
    lam = float(np.float32(c.lam))
    u = po._fgs_pass64(src.astype(np.float64), ch, np.float32(c.lam))
    C = ch.astype(np.float64)
    a = np.zeros_like(C)
    a[:, 1:] = lam * C[:, :-1]
    cc = lam * C
    res = (1 - a - cc) * u
    res[:, 1:] += a[:, 1:] * u[:, :-1]
    res[:, :-1] += cc[:, :-1] * u[:, 1:]
    assert np.abs(res - src).max() <= 1e-9 * max(1.0, np.abs(src).max()) * max(1.0, lam)


def test_oracle_defaults_are_unchanged_by_the_new_keywords():
    c = pc.SOLVER[10]
    dl, dr, g = pc.case_inputs(c)
    a = po.wls_filter(dl, g, dr, 0, 16, 5, lam=8000, sigma_color=1.5)
    b, conf, q = po.wls_filter(dl, g, dr, 0, 16, 5, lam=8000, sigma_color=1.5, return_confidence=True, return_quotient=True,
                               radius=3, num_iter=3, lambda_attenuation=0.25, roll_off=0.001)
    np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(np.clip(np.rint(q), -32768, 32767).astype(np.int16), b[:, 16:])
    b2, conf2 = po.wls_filter(dl, g, dr, 0, 16, 5, lam=8000, sigma_color=1.5, return_confidence=True)
    np.testing.assert_array_equal(conf, conf2)
    assert (po.wls_filter(dl, g, dr, 0, 16, 5, num_iter=1) != a).any() and (po.wls_filter(dl, g, dr, 0, 16, 9, radius=3) == a).all()


def test_reflect101_of_the_oracle_for_rois_smaller_than_the_radius():
    """numpy's reflect padding past the array is the loop of BORDER_REFLECT_101 (p < 0 -> -p, p >= n -> 2n-2-p, repeated)."""
    def r101(p, n):
        if n == 1:
            return 0
        while p < 0 or p >= n:
            p = -p if p < 0 else 2 * n - 2 - p
        return p
    rng = np.random.default_rng(1)
    for (h, w), r in (((1, 1), 6), ((3, 2), 6), ((2, 3), 32), ((5, 40), 32)):
        d = rng.integers(-16, 90, (h, w))
        yy = [r101(y, h) for y in range(-r, h + r)]
        xx = [r101(x, w) for x in range(-r, w + r)]
        p = d[np.ix_(yy, xx)]
        k = 2 * r + 1
        want = np.array([[p[y:y + k, x:x + k].sum() for x in range(w)] for y in range(h)])
        got = po._box_mean_reflect101(d, r)
        np.testing.assert_array_equal(got, (want.astype(np.float64) * (1.0 / (k * k))).astype(np.float32))
