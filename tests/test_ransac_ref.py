"""The numpy restatement of the RANSAC contract (tests/ransac_ref.py) checked against itself and against known answers: no GPU.
The GPU tests (tests/test_ransac_gpu.py) compare the device with this restatement, so what is checked here is that the
restatement means what DESIGN.md says: the sampler's values, the literal and the vectorised form agreeing, a planted motion
coming back, the stop rule's corner cases, and that the loosely compared hypotheses stay under 2 % in every GPU case."""
import functools

import numpy as np
import pytest

from tests import ransac_ref as rr


def test_sampler_known_answers():
    # splitmix64 from state 0: the first output is mix(GOLD), a published value
    assert rr.mix(rr.GOLD) == 0xE220A8397B1DCDAF
    assert rr.mix(2 * rr.GOLD) == 0x6E789E6AA1B965F4
    # (seed, h, j, M) -> index: mix's high word scaled to [0, M)
    for seed, h, j, m in [(0, 0, 0, 600), (0, 0, 1, 600), (7, 1234567, 2, 2000), (2 ** 64 - 1, 2 ** 31 - 2, 3, 2 ** 31 - 1), (5, 9, 0, 3)]:
        u = rr.mix(seed + rr.GOLD * (8 * h + j + 1))
        want = ((u >> 32) * m) >> 32
        assert rr.sample_index(seed, h, j, m) == want and 0 <= want < m
    assert rr.sample_index(0, 0, 0, 600) == (0xE220A839 * 600) >> 32 == 529
    assert rr.sample_index(0, 0, 1, 1 << 20) == 0x6E789E6A >> 12 == 452489
    assert rr.sample_index(7, 1234567, 2, 2000) == 628 and rr.sample_index(2 ** 64 - 1, 2 ** 31 - 2, 3, 2 ** 31 - 1) == 1328242606
    # the vectorised sampler wraps as the integers do, at the top of the h range too
    for seed, h0, n, m in [(0, 0, 3, 600), (7, 2147000001, 4, 2000), (2 ** 64 - 1, 2 ** 31 - 65, 3, 2 ** 31 - 1)]:
        got = rr.samples(seed, h0, 64, n, m)
        want = [[rr.sample_index(seed, h0 + i, j, m) if j < n else -1 for j in range(4)] for i in range(64)]
        assert np.array_equal(got, np.array(want))


def test_umeyama_is_the_least_squares_rigid_motion():
    rng = np.random.default_rng(3)
    s = rng.uniform(0, 1, (5, 4, 3))
    r = rr.rotation([0.3, -1.0, 0.5], 2.1)
    t = s @ r.T + [0.1, 0.2, -0.3]
    tm, sv = rr.umeyama(s, t)
    assert np.abs(tm[:, :, :3] - r).max() < 1e-12 and np.abs(tm[:, :, 3] - [0.1, 0.2, -0.3]).max() < 1e-12
    assert (sv[:, 0] >= sv[:, 1]).all() and (sv[:, 1] >= sv[:, 2]).all()
    # a mirrored target still gives a proper rotation
    tm, _ = rr.umeyama(s, t * [1, 1, -1])
    assert np.allclose(np.linalg.det(tm[:, :, :3]), 1.0)


@functools.lru_cache(maxsize=None)
def _ref(name):
    src, tgt, corres, kw = rr.parity_case(name)
    return src, tgt, corres, kw, rr.hypotheses(src, tgt, corres, **kw)


@pytest.mark.parametrize("name", ["planted257", "n4", "no_checker", "run+1"])
def test_literal_equals_vectorised(name):
    src, tgt, corres, kw, hy = _ref(name)
    kw1 = {k: v for k, v in kw.items() if k not in ("h0", "count")}
    for i in range(0, kw["count"], 7)[:120]:
        c, flags, tm, cnt, err = rr.hypothesis_literal(src, tgt, corres, kw["h0"] + i, **kw1)
        assert c == list(hy["samples"][i, :kw["n"]]) and flags == hy["flags"][i]
        assert cnt == hy["inliers"][i] or hy["sens_pairs"][i] > 0
        if flags & 1 and not hy["ill"][i]:
            assert np.abs(tm - hy["T"][i]).max() < 1e-12
            assert abs(err - hy["err2"][i]) <= 1e-12 * max(err, 1e-300) or hy["sens_pairs"][i] > 0


@pytest.mark.parametrize("name,stop", [("planted600", 137), ("planted2000", 765)])
def test_planted_motion_is_recovered(name, stop):
    m, ni, n, edge, cd, _, count = rr.PARITY_CASES[name]
    src, tgt, corres, t_true, planted = rr.planted_case(m, ni, seed=m + n)
    res = rr.run(src, tgt, corres, rr.MAX_DIST, n, edge, cd, max_iteration=count, confidence=0.999, seed=0)
    assert np.array_equal(res["mask"], planted) and res["inliers"] == ni
    assert np.abs(res["T"] - t_true).max() < 0.005                   # 2 mm noise over a unit cube
    assert res["iterations"] == stop < count and 0 <= res["best_hypothesis"] < stop
    lit = rr.run(src, tgt, corres, rr.MAX_DIST, n, edge, cd, max_iteration=count, confidence=0.999, seed=0, literal=True)
    for k in ("iterations", "validated", "best_hypothesis", "inliers"):
        assert lit[k] == res[k]
    assert np.abs(lit["T"] - res["T"]).max() < 1e-12


def test_stop_rule():
    src, tgt, corres, _, _ = rr.planted_case(600, 220, seed=603)
    kw = dict(max_dist=rr.MAX_DIST, n=3, edge=0.9, checker_distance=rr.MAX_DIST, seed=0)
    early = rr.run(src, tgt, corres, max_iteration=3000, confidence=0.999, **kw)
    full = rr.run(src, tgt, corres, max_iteration=3000, confidence=1.0, **kw)
    assert full["iterations"] == 3000 and early["iterations"] < 3000
    assert full["inliers"] >= early["inliers"] and full["validated"] >= early["validated"]
    for it in (1, 5, 137, 138):
        r = rr.run(src, tgt, corres, max_iteration=it, confidence=0.999, **kw)
        assert r["iterations"] <= it and r["best_hypothesis"] < it
    # every pair an exact inlier: hypothesis 0 has fitness 1, est_k = 0, and the walk stops at h = 1
    exact = src @ rr.rotation([0, 0, 1], 0.5).T
    ident = np.stack([np.arange(600), np.arange(600)], 1).astype(np.int32)
    r = rr.run(src, exact, ident, max_iteration=1000, confidence=0.999, **kw)
    assert r["iterations"] == 1 and r["best_hypothesis"] == 0 and r["fitness"] == 1.0
    assert rr.est_k(1.0, 3, 0.999, 50) == 0 and rr.est_k(0.5, 3, 1.0, 50) == 50 and rr.est_k(1e-200, 3, 0.999, 50) == 50
    assert rr.est_k(0.5, 3, 0.999, 10 ** 6) == 52                   # ceil(log(0.001) / log1p(-0.125)) = ceil(51.73)
    # nothing survives: identity, no best
    none = rr.run(src, tgt[::-1].copy(), ident, max_iteration=300, confidence=0.999, max_dist=rr.MAX_DIST, n=3, edge=0.999,
                  checker_distance=rr.MAX_DIST, seed=0)
    assert none["best_hypothesis"] == -1 and none["fitness"] == 0 and np.array_equal(none["T"], np.eye(4)) and none["iterations"] == 300


@pytest.mark.parametrize("name", sorted(rr.PARITY_CASES))
def test_loose_share_stays_under_the_cap(name):
    """Ill-conditioned plus sensitive hypotheses are under 2 % of those compared, so the loose branch of the GPU comparison cannot
    hide a failure.  With M pairs a share of about 3 / M of the samples repeats an index (rank 1), so the cap can only hold for
    M >= 150: the one smaller case, M = 3 = ransac_n, instead requires that its ill-conditioned samples are EXACTLY those with a
    repeated index (21 of 27 by count), which the GPU test then checks for finite, orthonormal transforms."""
    _, _, _, kw, hy = _ref(name)
    loose = hy["ill"] | (hy["sens_flags"] > 0) | (hy["sens_pairs"] > 0)
    c = hy["samples"][:, :kw["n"]]
    if name == "m3":
        repeated = np.array([len(set(r)) < 3 for r in c.tolist()])
        assert np.array_equal(loose, repeated) and 0.1 < 1 - repeated.mean() < 0.35
        return
    assert loose.sum() <= 0.02 * kw["count"], (loose.sum(), kw["count"])
    if name == "coincident":                                         # the case is there for rank 0 and rank 1 samples: it has both
        in_cluster = (c < rr.COINCIDENT_PAIRS).sum(1)
        assert (in_cluster == 3).any() and (in_cluster == 2).any()
    if kw["edge"] and kw["checker_distance"]:                       # the estimator does real work: both checkers reject, some pass
        assert 0 < (hy["flags"] == 3).sum() < (hy["flags"] & 1).sum() < kw["count"]
