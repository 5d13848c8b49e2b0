"""The horizontal scan's own output, the volume L_left + L_right, entry by entry against a numpy reference.

The final maps are a weak check of this kernel on small images: with C2's parameters most pixels right of column D are
invalid there, and a wrong sum can hide behind an invalid pixel.  The volume has no such gaps.  Reference: the oracle's cost
rows pushed through the path recurrence (`step` of tests/sgbm_numpy_ref.py) forward and backward along every row, summed.
No tolerance, no excluded entries.  Path values stay far inside int16 for these inputs (sums within about +-7 400; every case
asserts it), so neither wrap nor clipping enters the comparison."""
import numpy as np
import pytest

from tests.sgbm_numpy_ref import step

pytestmark = pytest.mark.gpu

C2_KW = dict(minDisparity=0, blockSize=5, P1=600, P2=2400, disp12MaxDiff=1, uniquenessRatio=15,
             speckleWindowSize=0, speckleRange=2, preFilterCap=63)

# W1 = W - D (minDisparity 0): no full 16-column segment, then 1 to 8 full segments with and without tail columns, so that
# every position of the buffer rotation and of the round pairing is an end case; H: full and partial last waves (4 rows per
# wave); D: the unpadded and the padded 128-slot layouts.
GRID = [(w1, h, d) for d in (128, 112, 96) for h in (1, 3, 4, 5, 8, 9)
        for w1 in (7, 15, 16, 17, 32, 47, 48, 64, 65, 80, 81, 96, 112, 129)]
# two larger maps, and one case each for the layouts that share the kernel template (32, 64 and 256 slots)
EXTRA = [(1000, 41, 128), (333, 23, 96), (97, 9, 32), (130, 10, 64), (75, 6, 256)]


def reference_sum(C, P1, P2):
    """C: [H, W1, D] costs -> L_left + L_right, int64 [H, W1, D]."""
    H, W1, D = C.shape
    C = C.astype(np.int64)
    out = np.zeros((H, W1, D), np.int64)
    for y in range(H):
        prev, pm = np.zeros(D, np.int64), 0
        for x in range(W1):
            prev, pm = step(C[y, x], prev, pm, P1, P2)
            out[y, x] = prev
        prev, pm = np.zeros(D, np.int64), 0
        for x in range(W1 - 1, -1, -1):
            prev, pm = step(C[y, x], prev, pm, P1, P2)
            out[y, x] += prev
    return out


@pytest.mark.parametrize("W1,H,D", GRID + EXTRA)
def test_sum_volume_equals_reference(r3d, synth, W1, H, D):
    from oracle import sgbm_oracle as so
    L, R, _ = synth.stereo_pair(W1 + D, H, D, seed=1000 * D + 10 * W1 + H)
    m = r3d.StereoSGBM_create(numDisparities=D, mode=r3d.STEREO_SGBM_MODE_SGBM_3WAY, **C2_KW)
    m.compute(L, R)
    st = m.debug_fetch(want_cost=True, want_hsum=True, want_raw=False)
    C = so.cost_rows(L, R, so.make_params(numDisparities=D, **C2_KW), 0, 0, H)
    assert C.shape == (H, W1, D)
    np.testing.assert_array_equal(st["cost"], C)
    want = reference_sum(C, C2_KW["P1"], C2_KW["P2"])
    assert np.abs(want).max() < 32767                      # the int16 volume holds the reference without wrap
    np.testing.assert_array_equal(st["hsum"].astype(np.int64), want)


def test_c2_map_three_times_identical_sum_volume(r3d, synth):
    """The 8 MP C2 map computed three times in one process: map and sum volume identical each time (a race between the
    waves or launches of the scan would show as a difference)."""
    W, H, D = 3264, 2448, 128
    L, R, _ = synth.stereo_pair(W, H, D)
    m = r3d.StereoSGBM_create(numDisparities=D, mode=r3d.STEREO_SGBM_MODE_SGBM_3WAY, **C2_KW)
    disp0 = m.compute(L, R)
    hsum0 = m.debug_fetch(want_hsum=True, want_raw=False)["hsum"]
    assert hsum0.shape == (H, W - D, D) and hsum0.any()
    for _ in range(2):
        disp = m.compute(L, R)
        hsum = m.debug_fetch(want_hsum=True, want_raw=False)["hsum"]
        np.testing.assert_array_equal(disp, disp0)
        assert np.array_equal(hsum, hsum0)
        del hsum
