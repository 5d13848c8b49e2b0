"""GPU parity tests of SGBM MODE_HH: every map bit-exact against the restatement tests/sgbm_hh_ref.py, on both the raw
(LR-checked, pre-median) map of debug_fetch and the final map."""
import numpy as np
import pytest

from tests import sgbm_hh_ref as hh

pytestmark = pytest.mark.gpu

C2_KW = dict(minDisparity=0, blockSize=5, P1=600, P2=2400, disp12MaxDiff=1, uniquenessRatio=15,
             speckleWindowSize=0, speckleRange=2, preFilterCap=63)
D4_KW = dict(minDisparity=0, blockSize=5, P1=600, P2=2400, disp12MaxDiff=1, uniquenessRatio=10,
             speckleWindowSize=50, speckleRange=32, preFilterCap=63)


def _hh(r3d, D, kw):
    return r3d.StereoSGBM_create(numDisparities=D, mode=r3d.STEREO_SGBM_MODE_HH, **kw)


def _check(r3d, L, R, D, kw):
    m = _hh(r3d, D, kw)
    got = m.compute(L, R)
    want, want_raw = hh.compute(L, R, return_raw=True, numDisparities=D, **kw)
    np.testing.assert_array_equal(m.debug_fetch()["raw"], want_raw)
    np.testing.assert_array_equal(got, want)
    return got


def test_mode_constant_is_exported(r3d):
    assert r3d.STEREO_SGBM_MODE_HH == 1 and r3d.stereo_sgbm.STEREO_SGBM_MODE_HH == 1


@pytest.mark.parametrize("W,H,D,seed", [(96, 40, 16, 0), (200, 90, 32, 1), (333, 121, 64, 2), (640, 480, 16, 3),
                                        (512, 384, 64, 4), (500, 203, 128, 5), (700, 150, 256, 6), (301, 77, 48, 7),
                                        (420, 99, 112, 8), (600, 64, 160, 9),
                                        (60, 200, 32, 10), (150, 333, 16, 11), (17, 1, 16, 12), (18, 2, 16, 13),
                                        (33, 3, 32, 14), (70, 11, 32, 15), (19, 40, 16, 16)])
def test_bit_exact_vs_restatement(r3d, synth, W, H, D, seed):
    """The 3WAY shape grid plus H > W1 (tall and narrow), images a few rows tall and a matching range a few columns wide."""
    L, R, _ = synth.stereo_pair(W, H, D, seed=seed)
    got = _check(r3d, L, R, D, C2_KW)
    assert got.dtype == np.int16 and (got[:, :D] == -16).all()


def test_rig_resolution(r3d, synth):
    L, R, _ = synth.stereo_pair(960, 540, 128, seed=1)
    got = _check(r3d, L, R, 128, C2_KW)
    assert (got[:, 128:] >= 0).mean() > 0.8


@pytest.mark.parametrize("bs", [1, 3, 5, 7, 9, 11])
def test_block_sizes_with_reference_penalties(r3d, synth, bs):
    """P1 = 8*3*bs^2, P2 = 32*3*bs^2: from blockSize 7 on, S saturates at -32768 and the fold order decides the map."""
    D = 32
    L, R, _ = synth.stereo_pair(260, 110, D, seed=20 + bs)
    kw = dict(C2_KW, blockSize=bs, P1=8 * 3 * bs * bs, P2=32 * 3 * bs * bs)
    _check(r3d, L, R, D, kw)


def test_random_noise_flat_images_and_no_uniqueness(r3d):
    rng = np.random.default_rng(1)
    L = rng.integers(0, 256, (70, 180), dtype=np.uint8)
    R = rng.integers(0, 256, (70, 180), dtype=np.uint8)
    _check(r3d, L, R, 32, C2_KW)
    Z = np.full((50, 120), 77, np.uint8)                      # all costs tie: first minimum wins
    _check(r3d, Z, Z, 16, C2_KW)
    _check(r3d, Z, Z, 16, dict(C2_KW, uniquenessRatio=0))
    _check(r3d, L, R, 48, dict(C2_KW, uniquenessRatio=0, minDisparity=-9))


def test_right_matcher(r3d, synth):
    D = 64
    L, R, _ = synth.stereo_pair(400, 120, D, seed=21)
    left = _hh(r3d, D, C2_KW)
    right = r3d.createRightMatcher(left)
    assert right.getMode() == r3d.STEREO_SGBM_MODE_HH
    kw = dict(C2_KW, minDisparity=-D + 1, uniquenessRatio=0, disp12MaxDiff=1000000)
    np.testing.assert_array_equal(right.compute(R, L), hh.compute(R, L, numDisparities=D, **kw))


@pytest.mark.parametrize("W,H,D,seed", [(320, 240, 32, 0), (640, 480, 128, 1)])
def test_depth4_family_with_speckles(r3d, synth, W, H, D, seed):
    L, R, _ = synth.stereo_pair(W, H, D, seed=seed, noise=6.0)
    got = _check(r3d, L, R, D, D4_KW)
    assert (got != hh.compute(L, R, numDisparities=D, **dict(D4_KW, speckleWindowSize=0))).any()


def test_set_mode_on_a_live_matcher(r3d, synth):
    from oracle import sgbm_oracle as so
    D = 64
    L, R, _ = synth.stereo_pair(320, 100, D, seed=12)
    m = r3d.StereoSGBM_create(numDisparities=D, mode=r3d.STEREO_SGBM_MODE_SGBM_3WAY, **C2_KW)
    m.setMode(1)
    np.testing.assert_array_equal(m.compute(L, R), hh.compute(L, R, numDisparities=D, **C2_KW))
    m.setMode(2)
    np.testing.assert_array_equal(m.compute(L, R), so.compute(L, R, so.make_params(numDisparities=D, **C2_KW), nthreads=4))


def test_device_and_batch_entry_points_equal_compute(r3d, synth):
    D = 64
    pairs = [synth.stereo_pair(384, 200, D, seed=40 + i)[:2] for i in range(4)]
    m = _hh(r3d, D, C2_KW)
    single = [m.compute(a, b) for a, b in pairs]
    for got, want in zip(m.compute_batch([p[0] for p in pairs], [p[1] for p in pairs]), single):
        np.testing.assert_array_equal(got, want)
    L, R = pairs[0]
    H, W = L.shape
    ctx = m.context
    d_l, d_r, d_d = ctx.to_device(L), ctx.to_device(R), ctx.alloc(W * H * 2)
    try:
        m.compute_device(d_l, d_r, W, H, W, d_d)
        ctx.sync()
        got = np.empty((H, W), np.int16)
        ctx.d2h(got, d_d)
    finally:
        for p in (d_l, d_r, d_d):
            ctx.free(p)
    np.testing.assert_array_equal(got, single[0])
    np.testing.assert_array_equal(single[0], hh.compute(L, R, numDisparities=D, **C2_KW))


def test_wls_chain(r3d, synth):
    """left HH + right HH + createDisparityWLSFilter (which re-configures the left matcher: uniqueness 0, disp12 1e6, no
    speckles) against the WLS oracle run on the restatement's two maps."""
    from oracle import prepost_oracle as po
    D, bs = 64, 5
    L, R, _ = synth.stereo_pair(400, 150, D, seed=31)
    left = r3d.StereoSGBM_create(numDisparities=D, mode=r3d.STEREO_SGBM_MODE_HH, **dict(C2_KW, speckleWindowSize=50))
    right = r3d.createRightMatcher(left)
    wls = r3d.createDisparityWLSFilter(left)
    wls.setLambda(8000)
    wls.setSigmaColor(1.5)
    dl, dr = left.compute(L, R), right.compute(R, L)
    kl = dict(C2_KW, uniquenessRatio=0, disp12MaxDiff=1000000, speckleWindowSize=0)
    kr = dict(kl, minDisparity=-D + 1)
    want_l, want_r = hh.compute(L, R, numDisparities=D, **kl), hh.compute(R, L, numDisparities=D, **kr)
    np.testing.assert_array_equal(dl, want_l)
    np.testing.assert_array_equal(dr, want_r)
    filt = wls.filter(dl, L, None, dr)
    d = np.abs(filt.astype(int) - po.wls_filter(want_l, L, want_r, 0, D, bs, lam=8000, sigma_color=1.5).astype(int))
    assert d.max() <= 1 and (d > 0).mean() <= 1e-3


def test_refused_modes_and_envelope_are_loud(r3d):
    L = np.zeros((40, 100), np.uint8)
    for mode in (0, 3):
        with pytest.raises(r3d.R3DError, match="HH \\(1\\)"):
            r3d.StereoSGBM_create(numDisparities=16, blockSize=5, mode=mode).compute(L, L)
    with pytest.raises(r3d.R3DError):
        _hh(r3d, 24, C2_KW).compute(L, L)                                          # not a multiple of 16
    with pytest.raises(r3d.R3DError):
        _hh(r3d, 16, dict(C2_KW, P2=20000)).compute(L, L)                          # P2 > 16383
    with pytest.raises(r3d.R3DError):
        _hh(r3d, 16, dict(C2_KW, blockSize=11, preFilterCap=127)).compute(L, L)    # block cost may pass 32767
    saw = ((np.arange(200) % 32) * 8).astype(np.uint8)[None, :].repeat(60, 0)   # block cost 19 360 at blockSize 11 (oracle)
    with pytest.raises(r3d.R3DError, match="envelope"):                           # the tracked maximum passes 16383
        _hh(r3d, 16, dict(C2_KW, blockSize=11, preFilterCap=63)).compute(saw, 255 - saw)


def test_empty_matching_range_gives_all_invalid_map(r3d):
    L = np.random.default_rng(0).integers(0, 256, (12, 157), dtype=np.uint8)
    got = _hh(r3d, 144, dict(C2_KW, minDisparity=16, blockSize=11)).compute(L, L)
    assert (got == 15 * 16).all()
