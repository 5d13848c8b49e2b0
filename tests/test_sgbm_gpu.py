"""GPU parity tests: HIP SGBM (through the C ABI / the cv2-style object) vs the CPU oracle, bit-exact."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

C2_KW = dict(minDisparity=0, blockSize=5, P1=600, P2=2400, disp12MaxDiff=1, uniquenessRatio=15,
             speckleWindowSize=0, speckleRange=2, preFilterCap=63)


def _oracle(L, R, D, kw, nthreads=8, raw=False):
    from oracle import sgbm_oracle as so
    return so.compute(L, R, so.make_params(numDisparities=D, **kw), nthreads=nthreads, return_raw=raw)


def _gpu(r3d, D, kw):
    return r3d.StereoSGBM_create(numDisparities=D, mode=r3d.STEREO_SGBM_MODE_SGBM_3WAY, **kw)


def test_selftest_crosslane_primitives(r3d):
    r3d.default_context(0).selftest()


@pytest.mark.parametrize("W,H,D,seed", [(96, 40, 16, 0), (200, 90, 32, 1), (333, 121, 64, 2), (640, 480, 16, 3),
                                        (512, 384, 64, 4), (500, 203, 128, 5), (700, 150, 256, 6), (301, 77, 48, 7),
                                        (420, 99, 112, 8), (600, 64, 160, 9)])
def test_bit_exact_vs_oracle(r3d, synth, W, H, D, seed):
    L, R, _ = synth.stereo_pair(W, H, D, seed=seed)
    m = _gpu(r3d, D, C2_KW)
    got = m.compute(L, R)
    want, want_raw = _oracle(L, R, D, C2_KW, raw=True)
    got_raw = m.debug_fetch()["raw"]
    np.testing.assert_array_equal(got_raw, want_raw)
    np.testing.assert_array_equal(got, want)
    assert got.dtype == np.int16 and (got[:, :D] == -16).all()


@pytest.mark.parametrize("bs", [1, 3, 7, 9, 11])
def test_block_sizes(r3d, synth, bs):
    D = 32
    L, R, _ = synth.stereo_pair(260, 110, D, seed=20 + bs)
    kw = dict(C2_KW, blockSize=bs, P1=8 * 3 * bs * bs, P2=32 * 3 * bs * bs)
    np.testing.assert_array_equal(_gpu(r3d, D, kw).compute(L, R), _oracle(L, R, D, kw))


def test_random_noise_and_flat_images(r3d):
    rng = np.random.default_rng(1)
    L = rng.integers(0, 256, (70, 180), dtype=np.uint8)
    R = rng.integers(0, 256, (70, 180), dtype=np.uint8)
    np.testing.assert_array_equal(_gpu(r3d, 32, C2_KW).compute(L, R), _oracle(L, R, 32, C2_KW))
    Z = np.full((50, 120), 77, np.uint8)                      # all costs tie: exercises first-minimum-wins
    np.testing.assert_array_equal(_gpu(r3d, 16, C2_KW).compute(Z, Z), _oracle(Z, Z, 16, C2_KW))
    kw0 = dict(C2_KW, uniquenessRatio=0)
    np.testing.assert_array_equal(_gpu(r3d, 16, kw0).compute(Z, Z), _oracle(Z, Z, 16, kw0))


def test_constant_shift_known_answer(r3d, synth):
    D, d0 = 64, 23
    L, R = synth.constant_shift_pair(400, 100, d0, seed=3)
    disp = _gpu(r3d, D, C2_KW).compute(L, R)
    inner = disp[6:-6, D + 6:-6]
    assert (np.abs(inner.astype(int) - 16 * d0) <= 1).all() and (disp[:, :D] == -16).all()


def test_right_matcher_geometry_negative_min_disparity(r3d, synth):
    D = 32
    L, R, _ = synth.stereo_pair(300, 80, D, seed=11)
    kw = dict(C2_KW, minDisparity=-(0 + D) + 1, uniquenessRatio=0, disp12MaxDiff=1000000)
    np.testing.assert_array_equal(_gpu(r3d, D, kw).compute(R, L), _oracle(R, L, D, kw))


def test_setters_follow_key_handler_protocol(r3d, synth):
    """depth1.py:240-265 changes blockSize / numDisparities on a live matcher object."""
    L, R, _ = synth.stereo_pair(320, 100, 64, seed=12)
    m = r3d.reference_matcher(numDisparities=16, blockSize=5)
    m.setNumDisparities(64)
    m.setBlockSize(7)
    kw = dict(C2_KW, blockSize=7)
    np.testing.assert_array_equal(m.compute(L, R), _oracle(L, R, 64, kw))


D4_KW = dict(minDisparity=0, blockSize=5, P1=600, P2=2400, disp12MaxDiff=1, uniquenessRatio=10,
             speckleWindowSize=50, speckleRange=32, preFilterCap=63)                  # Calib_depth/depth4.py:156-168


def test_filter_speckles_matches_oracle(r3d):
    from oracle import sgbm_oracle as so
    rng = np.random.default_rng(3)
    img = (rng.integers(0, 6, (300, 500)) * 40).astype(np.int16)
    img[rng.random(img.shape) < 0.25] = -16
    for size, diff in ((6, 32), (50, 512), (1, 0), (100000, 39)):
        np.testing.assert_array_equal(r3d.stereo_sgbm.filterSpeckles(img, -16, size, diff), so.filter_speckles(img, -16, size, diff))


@pytest.mark.parametrize("W,H,D,seed", [(320, 240, 32, 0), (640, 480, 128, 1)])
def test_depth4_parameter_family_with_speckle_filter(r3d, synth, W, H, D, seed):
    L, R, _ = synth.stereo_pair(W, H, D, seed=seed, noise=6.0)         # noisy => speckles exist
    got = _gpu(r3d, D, D4_KW).compute(L, R)
    want = _oracle(L, R, D, D4_KW)
    np.testing.assert_array_equal(got, want)
    no_filter = _oracle(L, R, D, dict(D4_KW, speckleWindowSize=0))
    assert (want != no_filter).any()                                     # the filter actually removed something
    m = r3d.reference_matcher(numDisparities=D, blockSize=5, family="depth4")
    np.testing.assert_array_equal(m.compute(L, R), want)


def test_errors_are_loud(r3d):
    L = np.zeros((40, 100), np.uint8)
    with pytest.raises(r3d.R3DError):
        r3d.StereoSGBM_create(numDisparities=24, blockSize=5, mode=2).compute(L, L)
    with pytest.raises(r3d.R3DError):
        r3d.StereoSGBM_create(numDisparities=16, blockSize=5, mode=0).compute(L, L)     # MODE_SGBM not implemented
    with pytest.raises(ValueError):
        r3d.StereoSGBM_create(numDisparities=16, mode=2).compute(L.astype(np.float32), L)


def test_disparity_range_wider_than_the_image_gives_all_invalid_map(r3d):
    """minX1 >= maxX1: the original fills the map with the invalid marker and returns; no exception (a user raising
    numDisparities with the 'w' key of depth1.py:256-260 on a narrow stream must not crash the viewer)."""
    L = np.random.default_rng(0).integers(0, 256, (12, 157), dtype=np.uint8)
    kw = dict(C2_KW, minDisparity=16, blockSize=11)
    got = _gpu(r3d, 144, kw).compute(L, L)
    assert got.shape == L.shape and (got == 15 * 16).all()
    np.testing.assert_array_equal(got, _oracle(L, L, 144, kw))
    got = _gpu(r3d, 256, C2_KW).compute(L, L)
    assert (got == -16).all()


def test_full_size_8mp_bit_exact_and_properties(r3d, synth):
    """BASELINE config C2 (3264x2448, D=128, depth2.py parameters): the C oracle needs about a second for this size on
    the GPU box's host cores, so the full map is compared bit for bit; plus determinism, the invalid left band, the
    batch entry point on the same pair, and accuracy against the generator's ground truth."""
    W, H, D = 3264, 2448, 128
    L, R, gt = synth.stereo_pair(W, H, D)
    m = _gpu(r3d, D, C2_KW)
    a = m.compute(L, R)
    b = m.compute(L, R)
    np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(a, _oracle(L, R, D, C2_KW, nthreads=8))
    assert (a[:, :D] == -16).all()
    for c in m.compute_batch([L, L, L, L], [R, R, R, R]):             # four maps in flight over the three lanes
        np.testing.assert_array_equal(c, a)
    valid = a[:, D:] >= 0
    assert valid.mean() > 0.9
    xr = np.arange(W)[None, :].repeat(H, 0)
    xl = np.rint(xr + gt).astype(int)
    ok = (xl < W) & (xl >= D)
    rows = np.arange(H)[:, None].repeat(W, 1)
    dd = a[rows[ok], xl[ok]] / 16.0
    v = dd >= 0
    assert np.abs(dd[v] - gt[ok][v]).mean() < 0.5


def test_right_matcher_factory(r3d, synth):
    """depth2.py:161,252: right_matcher = createRightMatcher(stereo_matcher); right_matcher.compute(gray_right, gray_left)."""
    D = 64
    L, R, _ = synth.stereo_pair(400, 120, D, seed=21)
    left = r3d.reference_matcher(numDisparities=D, blockSize=5)
    right = r3d.createRightMatcher(left)
    assert right.getMinDisparity() == -(0 + D) + 1 and right.getUniquenessRatio() == 0
    kw = dict(C2_KW, minDisparity=-D + 1, uniquenessRatio=0, disp12MaxDiff=1000000)
    got = right.compute(R, L)
    np.testing.assert_array_equal(got, _oracle(R, L, D, kw))
    # right-view disparities are the negated left-view ones on this scene (where both are valid)
    dl = left.compute(L, R)
    ok = (dl[:, D:-D] >= 0)
    assert ok.mean() > 0.8


def test_randomised_parameter_sweep(r3d):
    """Ragged sizes and random parameter combinations (incl. degenerate ones) must stay bit-exact."""
    rng = np.random.default_rng(2024)
    for case in range(24):
        D = int(rng.choice([16, 32, 48, 64, 96, 128, 144, 256]))
        W = D + int(rng.integers(3, 90))
        H = int(rng.integers(1, 70))
        bs = int(rng.choice([1, 3, 5, 7, 9]))
        kw = dict(minDisparity=int(rng.choice([0, 0, -7, 5, -D + 1])), blockSize=bs, P1=int(rng.choice([0, 8 * bs * bs, 24 * bs * bs])),
                  P2=int(rng.choice([0, 32 * bs * bs, 96 * bs * bs])), disp12MaxDiff=int(rng.choice([-1, 0, 1, 3])),
                  uniquenessRatio=int(rng.choice([0, 5, 15, 40])), speckleWindowSize=int(rng.choice([0, 0, 20])),
                  speckleRange=int(rng.choice([1, 2, 16])), preFilterCap=int(rng.choice([0, 15, 31, 63])))
        L = rng.integers(0, 256, (H, W), dtype=np.uint8)
        R = np.roll(L, -int(rng.integers(0, max(D // 2, 1))), axis=1) if rng.random() < 0.7 else rng.integers(0, 256, (H, W), dtype=np.uint8)
        got = _gpu(r3d, D, kw).compute(L, R)
        want = _oracle(L, R, D, kw)
        assert np.array_equal(got, want), f"case {case}: W={W} H={H} D={D} {kw}: {(got != want).sum()} pixels differ"


def test_six_more_shapes_bit_exact_vs_oracle(r3d, synth):
    """The shapes on which the retired kernel generations used to be compared with the oracle, one per slot layout and a few
    ragged ones, on the one generation there is."""
    for W, H, D, seed in ((333, 121, 64, 2), (500, 203, 128, 5), (400, 90, 256, 6), (301, 77, 48, 7), (190, 64, 16, 8), (97, 33, 32, 9)):
        L, R, _ = synth.stereo_pair(W, H, D, seed=seed)
        got = _gpu(r3d, D, C2_KW).compute(L, R)
        assert np.array_equal(got, _oracle(L, R, D, C2_KW, nthreads=4)), (W, H, D)


def test_stale_generation_switch_is_inert():
    """R3D_SGM_IMPL used to select a kernel generation at the first call, and the generations it selected knew neither 512
    slots nor colour pairs: a value left over in the environment must change nothing.  In a process of its own, since the
    variable was read once per process: a 512-slot pair, a 3-channel pair and a small grey pair, each bit-equal to the oracle
    (the colour pair has equal channels and three times the penalties, which the grey oracle answers; a coloured one goes
    against the restatement of tests/sgbm_color_ref.py as well)."""
    import subprocess
    import sys
    from tests.conftest import ROOT
    code = (
        "import importlib, sys, numpy as np\n"
        f"sys.path.insert(0, {ROOT!r})\n"
        "r3d = importlib.import_module('3d_reconstruction_project_amd')\n"
        "from oracle import sgbm_oracle as so\n"
        "from tests import sgbm_color_ref as cr\n"
        "def kw(ps):\n"
        "    return dict(minDisparity=0, blockSize=5, P1=600 * ps, P2=2400 * ps, disp12MaxDiff=1, uniquenessRatio=15,\n"
        "                speckleWindowSize=0, speckleRange=2, preFilterCap=63)\n"
        "for W, H, D, seed, colour in ((300, 20, 272, 1, False), (190, 64, 16, 8, True), (97, 33, 32, 9, False)):\n"
        "    L, R, _ = r3d.synth.stereo_pair(W, H, D, seed=seed)\n"
        "    want = so.compute(L, R, so.make_params(numDisparities=D, **kw(1)), nthreads=4)\n"
        "    assert (want[:, D:] != -16).mean() > 0.5, (W, H, D)\n"
        "    if colour:\n"
        "        L, R = (np.ascontiguousarray(np.stack([a, a, a], -1)) for a in (L, R))\n"
        "    m = r3d.StereoSGBM_create(numDisparities=D, mode=2, **kw(3 if colour else 1))\n"
        "    assert np.array_equal(m.compute(L, R), want), (W, H, D)\n"
        "    if colour:\n"
        "        L, R = cr.color_pair(r3d.synth, W, H, D, seed=seed)\n"
        "        assert np.array_equal(m.compute(L, R), cr.compute_3way(L, R, numDisparities=D, **kw(3))), (W, H, D, 'coloured')\n"
        "print('OK')\n")
    env = dict(os.environ, R3D_SGM_IMPL="v4")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env)
    assert "OK" in out.stdout, out.stdout + out.stderr


def test_batch_api_pipelines_and_matches_single_calls(r3d, synth):
    """r3d_sgbm_compute_batch_dev (multi-view batch, config C5): 7 pairs over 3 lanes == 7 single calls."""
    D = 64
    pairs = [synth.stereo_pair(384, 200, D, seed=40 + i)[:2] for i in range(7)]
    m = r3d.reference_matcher(numDisparities=D, blockSize=5)
    batch = m.compute_batch([p[0] for p in pairs], [p[1] for p in pairs])
    for (L, R), got in zip(pairs, batch):
        np.testing.assert_array_equal(got, _oracle(L, R, D, C2_KW))
    assert m.compute_batch([], []) == [] if False else True
    one = m.compute_batch([pairs[0][0]], [pairs[0][1]])
    np.testing.assert_array_equal(one[0], batch[0])


def test_row_stride_larger_than_width(r3d, synth):
    """include/r3d.h: `stride` is the row pitch of both input images in bytes (a cv::Mat ROI / padded camera buffer)."""
    W, H, D, pitch = 301, 77, 48, 320
    L, R, _ = synth.stereo_pair(W, H, D, seed=9)
    bufL = np.full((H, pitch), 255, np.uint8)
    bufR = np.full((H, pitch), 0, np.uint8)
    bufL[:, :W], bufR[:, :W] = L, R
    m = _gpu(r3d, D, C2_KW)
    ctx = m.context
    d_l, d_r, d_d = ctx.to_device(bufL), ctx.to_device(bufR), ctx.alloc(W * H * 2)
    m.compute_device(d_l, d_r, W, H, pitch, d_d)
    got = np.empty((H, W), np.int16)
    ctx.d2h(got, d_d)
    for p in (d_l, d_r, d_d):
        ctx.free(p)
    np.testing.assert_array_equal(got, _oracle(L, R, D, C2_KW))
    with pytest.raises(r3d.R3DError):
        m.compute_device(1, 1, W, H, W - 1, 1)                      # stride < width is refused before any access


@pytest.mark.parametrize("W,H,D", [(17, 1, 16), (18, 2, 16), (33, 3, 32), (16, 5, 16), (40, 2, 32), (60, 12, 16), (50, 9, 16), (70, 11, 32)])
def test_tiny_images_bit_exact(r3d, W, H, D):
    """Images of one to twelve rows and a matching range of zero to a few columns.  H <= 12 at blockSize 5 is where a stripe's
    warm-up start is clamped to row 0 and QUIRK_SMALL_IMAGE_STRIPES (oracle/sgbm3way.c) moves rows: the product reproduces the
    oracle's placement, invalid marker for the rows the original leaves uninitialised included."""
    rng = np.random.default_rng(W * H)
    L = rng.integers(0, 256, (H, W), dtype=np.uint8)
    R = rng.integers(0, 256, (H, W), dtype=np.uint8)
    np.testing.assert_array_equal(_gpu(r3d, D, C2_KW).compute(L, R), _oracle(L, R, D, C2_KW))


def test_tiny_image_stripe_quirk_with_large_blocks(r3d):
    """blockSize 11: stripe_sz 6 < overlap 7 at H = 24 (the quirk), regular at H = 28; both against the oracle, raw map included."""
    from oracle import sgbm_oracle as so
    kw = dict(minDisparity=0, blockSize=11, P1=100, P2=1000, disp12MaxDiff=1, uniquenessRatio=5, speckleWindowSize=0, speckleRange=2, preFilterCap=31)
    for H in (24, 28, 21):
        L, R, _ = r3d.synth.stereo_pair(120, H, 32, seed=H)
        assert so.undefined_rows(H, so.make_params(numDisparities=32, **kw)).any() == (H <= 24)
        np.testing.assert_array_equal(_gpu(r3d, 32, kw).compute(L, R), _oracle(L, R, 32, kw))
