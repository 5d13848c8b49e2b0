"""GPU parity tests of StereoSGBM on 3-channel pairs, both modes: every comparison exact, against the restatement
tests/sgbm_color_ref.py (block cost summed over the channels, then the grey algorithm) and, through the equal-channels rule,
against the frozen C oracle."""
import ctypes

import numpy as np
import pytest

from tests import sgbm_color_ref as cr

pytestmark = pytest.mark.gpu

SHAPES = [(200, 70, 32), (333, 121, 48), (300, 60, 128), (420, 50, 160), (600, 40, 272)]


def _kw(bs, minD=0, pscale=3, **extra):
    return dict(dict(minDisparity=minD, blockSize=bs, P1=8 * pscale * bs * bs, P2=32 * pscale * bs * bs, disp12MaxDiff=1,
                     uniquenessRatio=15, speckleWindowSize=0, speckleRange=2, preFilterCap=63), **extra)


D4 = dict(uniquenessRatio=10, speckleWindowSize=50, speckleRange=32)     # the depth4 family


def _gpu(r3d, D, kw, mode="3way"):
    mode = {"3way": r3d.STEREO_SGBM_MODE_SGBM_3WAY, "hh": r3d.STEREO_SGBM_MODE_HH}[mode]
    return r3d.StereoSGBM_create(numDisparities=D, mode=mode, **kw)


def _ref(mode, L, R, D, kw):
    """(final, raw) of the restatement; its own map must have something to compare."""
    fn = cr.compute_3way if mode == "3way" else cr.compute_hh
    want, want_raw = fn(L, R, return_raw=True, numDisparities=D, **kw)
    minD = kw["minDisparity"]
    assert (want[:, D + max(minD, 0):] != (minD - 1) * 16).mean() > 0.5, "the reference map is mostly invalid"
    return want, want_raw


def _check(r3d, mode, L, R, D, kw):
    m = _gpu(r3d, D, kw, mode)
    got = m.compute(L, R)
    want, want_raw = _ref(mode, L, R, D, kw)
    np.testing.assert_array_equal(m.debug_fetch()["raw"], want_raw)
    np.testing.assert_array_equal(got, want)
    assert got.dtype == np.int16 and got.shape == L.shape[:2]


def _grey3(a):
    return np.ascontiguousarray(np.stack([a, a, a], -1))


# ---- 1: the summed cost volume, every entry
@pytest.mark.parametrize("mode", ["3way", "hh"])
@pytest.mark.parametrize("W,H,D,bs,minD", [s + (bs, 0) for s in SHAPES for bs in (5, 3)] + [(300, 60, 128, 5, -5)])
def test_cost_volume_is_the_sum_over_the_channels(r3d, synth, W, H, D, bs, minD, mode):
    """Several column tiles, several 16-row bands (H = 121 on few tiles), every slot layout but 512 padded or full."""
    L, R = cr.color_pair(synth, W, H, D, seed=W)
    kw = _kw(bs, minD)
    m = _gpu(r3d, D, kw, mode)
    m.compute(L, R)
    np.testing.assert_array_equal(m.debug_fetch(want_cost=True, want_raw=False)["cost"],
                                  cr.block_cost(L, R, dict(kw, numDisparities=D), 0, 0, H))


# ---- 2: maps, both modes
@pytest.mark.parametrize("mode", ["3way", "hh"])
@pytest.mark.parametrize("W,H,D", SHAPES)
def test_maps_equal_the_restatement(r3d, synth, W, H, D, mode):
    L, R = cr.color_pair(synth, W, H, D, seed=W + 1)
    _check(r3d, mode, L, R, D, _kw(5, -5 if D == 128 else 0))


@pytest.mark.parametrize("mode", ["3way", "hh"])
@pytest.mark.parametrize("bs,cap", [(1, 63), (3, 63), (5, 63), (7, 31)])
def test_block_sizes(r3d, synth, bs, cap, mode):
    """blockSize 7 with preFilterCap 31: 3 * 49 * 125 = 18375 > 16383, the tracked-maximum path; this pair stays inside."""
    L, R = cr.color_pair(synth, 200, 70, 32, seed=3)
    _check(r3d, mode, L, R, 32, _kw(bs, preFilterCap=cap))


@pytest.mark.parametrize("mode", ["3way", "hh"])
def test_depth4_family_with_speckles(r3d, synth, mode):
    L, R = cr.color_pair(synth, 333, 121, 48, seed=9)
    _check(r3d, mode, L, R, 48, _kw(5, **D4))


# ---- 3: metamorphic, against the frozen C oracle (stripe-top rows, tiny-image quirk)
@pytest.mark.parametrize("bs", [3, 5])
@pytest.mark.parametrize("W,H,D", [(200, 70, 32), (640, 480, 16), (100, 10, 16)])
def test_equal_channels_with_three_times_the_penalties_equal_the_grey_oracle(r3d, synth, W, H, D, bs):
    from oracle import sgbm_oracle as so
    L, R, _ = synth.stereo_pair(W, H, D, seed=5)
    got = _gpu(r3d, D, _kw(bs, pscale=3, **D4)).compute(_grey3(L), _grey3(R))
    want = so.compute(L, R, so.make_params(numDisparities=D, **_kw(bs, pscale=1, **D4)), nthreads=4)
    np.testing.assert_array_equal(got, want)
    assert (want[:, D:] != -16).mean() > 0.5


@pytest.mark.parametrize("mode", ["3way", "hh"])
def test_channel_order_does_not_matter(r3d, synth, mode):
    L, R = cr.color_pair(synth, 200, 70, 32, seed=3)
    m = _gpu(r3d, 32, _kw(5), mode)
    a = m.compute(L, R)
    for perm in ([2, 1, 0], [1, 2, 0]):
        np.testing.assert_array_equal(m.compute(L[:, :, perm], R[:, :, perm]), a)     # non-contiguous views included
    assert (a[:, 32:] != -16).mean() > 0.5


# ---- 4: entry points
def _device_call(m, L, R, **kw):
    H, W = L.shape[:2]
    ctx = m.context
    d_l, d_r, d_d = ctx.to_device(L), ctx.to_device(R), ctx.alloc(W * H * 2)
    try:
        m.compute_device(d_l, d_r, W, H, L.strides[0], d_d, **kw)
        ctx.sync()
        got = np.empty((H, W), np.int16)
        ctx.d2h(got, d_d)
    finally:
        for p in (d_l, d_r, d_d):
            ctx.free(p)
    return got


@pytest.mark.parametrize("mode", ["3way", "hh"])
def test_batch_and_device_entry_points_equal_compute(r3d, synth, mode):
    D, W, H = 48, 333, 121
    pairs = [cr.color_pair(synth, W, H, D, seed=40 + i) for i in range(4)]
    m = _gpu(r3d, D, _kw(5), mode)
    single = [m.compute(a, b) for a, b in pairs]
    assert any((single[0] != s).any() for s in single[1:])
    for got, want in zip(m.compute_batch([p[0] for p in pairs], [p[1] for p in pairs]), single):
        np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(_device_call(m, *pairs[1], channels=3), single[1])
    # a batch with done_events on device pointers
    ctx = m.context
    dl = [ctx.to_device(p[0]) for p in pairs]
    dr = [ctx.to_device(p[1]) for p in pairs]
    dd = [ctx.alloc(W * H * 2) for _ in pairs]
    evs = [ctx.event() for _ in pairs]
    try:
        m.compute_batch_device(dl, dr, W, H, 3 * W, dd, done_events=evs, channels=3)
        for ev in evs:
            ctx.wait_event(ev)
        ctx.sync()
        for d, want in zip(dd, single):
            got = np.empty((H, W), np.int16)
            ctx.d2h(got, d)
            np.testing.assert_array_equal(got, want)
    finally:
        for q in dl + dr + dd:
            ctx.free(q)
        for ev in evs:
            ctx.call("r3d_event_destroy", ctypes.c_void_p(ev))


@pytest.mark.parametrize("mode", ["3way", "hh"])
def test_rows_wider_than_the_pixels(r3d, synth, mode):
    """stride > 3 * width (odd, so rows start at every alignment): the bytes between the rows are never read as pixels."""
    D, W, H = 32, 201, 71
    L, R = cr.color_pair(synth, W, H, D, seed=6)
    m = _gpu(r3d, D, _kw(5), mode)
    want = m.compute(L, R)
    stride = 3 * W + 7
    wide = [np.full((H, stride), 255 * i, np.uint8) for i in (0, 1)]
    for buf, img in zip(wide, (L, R)):
        buf[:, :3 * W] = img.reshape(H, 3 * W)
    ctx = m.context
    d_l, d_r, d_d = ctx.to_device(wide[0]), ctx.to_device(wide[1]), ctx.alloc(W * H * 2)
    try:
        m.compute_device(d_l, d_r, W, H, stride, d_d, channels=3)
        ctx.sync()
        got = np.empty((H, W), np.int16)
        ctx.d2h(got, d_d)
        with pytest.raises(r3d.R3DError, match="stride"):
            m.compute_device(d_l, d_r, W, H, 3 * W - 1, d_d, channels=3)
    finally:
        for q in (d_l, d_r, d_d):
            ctx.free(q)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(want, _ref(mode, L, R, D, _kw(5))[0])


def test_one_channel_through_the_new_entry_points_equals_the_grey_calls(r3d, synth):
    D, W, H = 48, 333, 121
    pairs = [synth.stereo_pair(W, H, D, seed=50 + i)[:2] for i in range(4)]
    m = _gpu(r3d, D, _kw(5))
    ctx, p, vp = m.context, m.params_struct(), ctypes.c_void_p
    L, R = pairs[0]
    old, new = np.empty((H, W), np.int16), np.empty((H, W), np.int16)
    ctx.call("r3d_sgbm_compute", ctypes.byref(p), L.ctypes.data_as(vp), R.ctypes.data_as(vp), W, H, W, old.ctypes.data_as(vp))
    ctx.call("r3d_sgbm_compute_cn", ctypes.byref(p), L.ctypes.data_as(vp), R.ctypes.data_as(vp), W, H, W, 1, new.ctypes.data_as(vp))
    np.testing.assert_array_equal(new, old)
    np.testing.assert_array_equal(m.compute(L, R), old)
    np.testing.assert_array_equal(_device_call(m, L, R, channels=1), old)
    dl = [ctx.to_device(a) for a, _ in pairs]
    dr = [ctx.to_device(b) for _, b in pairs]
    dd = [ctx.alloc(W * H * 2) for _ in range(2 * len(pairs))]
    arr = vp * len(pairs)
    try:
        ctx.call("r3d_sgbm_compute_batch_dev", ctypes.byref(p), len(pairs), arr(*dl), arr(*dr), W, H, W, arr(*dd[:4]))
        ctx.call("r3d_sgbm_compute_batch_cn_dev", ctypes.byref(p), len(pairs), arr(*dl), arr(*dr), W, H, W, 1, arr(*dd[4:]), None)
        ctx.sync()
        for i in range(len(pairs)):
            a, b = np.empty((H, W), np.int16), np.empty((H, W), np.int16)
            ctx.d2h(a, dd[i])
            ctx.d2h(b, dd[4 + i])
            np.testing.assert_array_equal(b, a)
            np.testing.assert_array_equal(a, m.compute(*pairs[i]))
    finally:
        for q in dl + dr + dd:
            ctx.free(q)
    for cn in (0, 2, 4):
        with pytest.raises(r3d.R3DError, match="BADARG"):
            ctx.call("r3d_sgbm_compute_cn", ctypes.byref(p), L.ctypes.data_as(vp), R.ctypes.data_as(vp), W // 4, H, W, cn,
                     new.ctypes.data_as(vp))


# ---- 5: the chain of the reference's frame loop, without cvtColor
@pytest.mark.parametrize("mode", ["3way", "hh"])
def test_wls_chain_with_colour_views(r3d, synth, mode):
    """Left colour matcher, createRightMatcher, WLS guided by the colour left view: both maps exact, the filtered map within
    the bound of tests/test_sgbm_hh_gpu.py::test_wls_chain (1 LSB, 1e-3 of the pixels)."""
    from oracle import prepost_oracle as po
    D, bs = 48, 5
    L, R = cr.color_pair(synth, 333, 121, D, seed=31)
    left = _gpu(r3d, D, _kw(bs, speckleWindowSize=50), mode)
    right = r3d.createRightMatcher(left)
    wls = r3d.createDisparityWLSFilter(left)
    wls.setLambda(8000)
    wls.setSigmaColor(1.5)
    dl, dr = left.compute(L, R), right.compute(R, L)
    kl = _kw(bs, uniquenessRatio=0, disp12MaxDiff=1000000)
    kr = dict(kl, minDisparity=-D + 1)
    fn = cr.compute_3way if mode == "3way" else cr.compute_hh
    want_l, want_r = fn(L, R, numDisparities=D, **kl), fn(R, L, numDisparities=D, **kr)
    np.testing.assert_array_equal(dl, want_l)
    np.testing.assert_array_equal(dr, want_r)
    assert (want_l[:, D:] != -16).mean() > 0.5
    filt = wls.filter(dl, L, None, dr)
    d = np.abs(filt.astype(int) - po.wls_filter(want_l, L, want_r, 0, D, bs, lam=8000, sigma_color=1.5).astype(int))
    assert d.max() <= 1 and (d > 0).mean() <= 1e-3


# ---- 6: errors
def test_errors_are_loud(r3d, synth):
    L, R = cr.color_pair(synth, 200, 70, 32, seed=3)
    m = _gpu(r3d, 32, _kw(5))
    with pytest.raises(ValueError):
        m.compute(L, R[:, :, 0])                                     # colour against grey
    with pytest.raises(ValueError):
        m.compute(L[:, :, 0], R)
    four = np.concatenate([L, L[:, :, :1]], -1)
    with pytest.raises(ValueError):
        m.compute(four, four)
    with pytest.raises(ValueError):
        m.compute(L[:, :, :2], R[:, :, :2])
    with pytest.raises(ValueError):
        m.compute(L.astype(np.float32), R.astype(np.float32))
    with pytest.raises(ValueError):
        m.compute_batch([L, L[:, :, 0]], [R, R[:, :, 0]])
    for mode in ("3way", "hh"):
        with pytest.raises(r3d.R3DError, match="envelope"):          # static: 3 * 81 * 189 = 45927 > 32767
            _gpu(r3d, 32, _kw(9), mode).compute(L, R)
        with pytest.raises(r3d.R3DError, match="envelope"):          # this pair: summed block cost 16923 > 16383 (CPU restatement)
            _gpu(r3d, 32, _kw(7), mode).compute(L, R)
    np.testing.assert_array_equal(m.compute(L, R), cr.compute_3way(L, R, numDisparities=32, **_kw(5)))   # and the context lives on


# ---- 7: one matcher object, grey then colour then grey
@pytest.mark.parametrize("mode", ["3way", "hh"])
def test_live_matcher_takes_grey_colour_grey(r3d, synth, mode):
    from oracle import sgbm_oracle as so
    from tests import sgbm_hh_ref as hh
    D, kw = 32, _kw(5)
    Lc, Rc = cr.color_pair(synth, 260, 90, D, seed=8)
    Lg, Rg, _ = synth.stereo_pair(300, 100, D, seed=8)       # larger than the colour pair, smaller than its three planes
    m = _gpu(r3d, D, kw, mode)
    if mode == "3way":
        grey = so.compute(Lg, Rg, so.make_params(numDisparities=D, **kw), nthreads=4)
    else:
        grey = hh.compute(Lg, Rg, numDisparities=D, **kw)
    colour, _ = _ref(mode, Lc, Rc, D, kw)
    np.testing.assert_array_equal(m.compute(Lg, Rg), grey)
    np.testing.assert_array_equal(m.compute(Lc, Rc), colour)
    np.testing.assert_array_equal(m.compute(Lg, Rg), grey)
    np.testing.assert_array_equal(m.compute(Lc, Rc), colour)
