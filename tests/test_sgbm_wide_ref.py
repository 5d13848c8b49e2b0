"""CPU checks that pin the yardsticks of the 512-slot layout (numDisparities 272 .. 512): the C oracle and its numpy
restatement agree there, the two MODE_HH restatements agree there, and the inputs really reach disparities >= 256 -- a map
whose winners all sit below 256 would pass on a matcher that dropped the upper half of the disparity vector.
H > 12 wherever tests/sgbm_numpy_ref.py is involved: it does not restate QUIRK_SMALL_IMAGE_STRIPES."""
import importlib

import numpy as np
import pytest

from tests import sgbm_hh_ref as hh
from tests import sgbm_numpy_ref as ref

synth = importlib.import_module("3d_reconstruction_project_amd.synth")

C2_KW = dict(minDisparity=0, blockSize=5, P1=600, P2=2400, disp12MaxDiff=1, uniquenessRatio=15,
             speckleWindowSize=0, speckleRange=2, preFilterCap=63)
WIDE_SHAPES = [(330, 40, 272, 1), (460, 37, 384, 2), (600, 52, 512, 3), (700, 33, 496, 4)]


@pytest.mark.parametrize("W,H,D,seed", WIDE_SHAPES)
def test_oracle_equals_numpy_restatement_above_256(W, H, D, seed):
    from oracle import sgbm_oracle as so
    L, R, _ = synth.stereo_pair(W, H, D, seed=seed)
    want, want_raw = so.compute(L, R, so.make_params(numDisparities=D, **C2_KW), nthreads=4, return_raw=True)
    got, got_raw = ref.compute(L, R, numDisparities=D, return_raw=True, **C2_KW)
    np.testing.assert_array_equal(got_raw, want_raw)
    np.testing.assert_array_equal(got, want)
    valid = want[want >= 0]
    assert valid.size > 0 and (valid >= 256 * 16).any() and (want[:, :D] == -16).all()


def test_oracle_equals_numpy_restatement_right_matcher_geometry():
    from oracle import sgbm_oracle as so
    D = 320
    L, R, _ = synth.stereo_pair(420, 30, D, seed=11)
    kw = dict(C2_KW, minDisparity=-D + 1, uniquenessRatio=0, disp12MaxDiff=1000000)
    want = so.compute(R, L, so.make_params(numDisparities=D, **kw), nthreads=4)
    np.testing.assert_array_equal(ref.compute(R, L, numDisparities=D, **kw), want)
    assert (want != (-D + 1 - 1) * 16).mean() > 0.1


def test_hh_restatements_agree_above_256():
    D, bs = 288, 3
    L, R, _ = synth.stereo_pair(300, 6, D, seed=5)
    kw = dict(C2_KW, numDisparities=D, blockSize=bs, P1=8 * bs * bs, P2=32 * bs * bs)
    a, ar = hh.compute(L, R, return_raw=True, **kw)
    b, br = hh.compute_literal(L, R, return_raw=True, **kw)
    np.testing.assert_array_equal(ar, br)
    np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("W,H,shift,D", [(460, 40, 300, 320), (640, 30, 500, 512)])
def test_constant_shift_above_256_is_recovered_by_both_yardsticks(W, H, shift, D):
    from oracle import sgbm_oracle as so
    L, R = synth.constant_shift_pair(W, H, shift)
    for disp in (so.compute(L, R, so.make_params(numDisparities=D, **C2_KW), nthreads=4), hh.compute(L, R, numDisparities=D, **C2_KW)):
        assert (disp[:, :D] == -16).all()
        assert (disp[8:-8, D + 8:-8] == 16 * shift).mean() >= 0.99
