"""CPU checks of tests/voxel_ref.py, the reference tests/test_voxel_edges_gpu.py compares the voxel kernels with: it agrees with
the oracle, its clouds have the member counts they were asked for, the order of summation is visible in its bits (the
precondition that makes an equality test sensitive to order), and continuing running sums frame by frame -- what the resident
model's table does -- gives the table of a full pass."""
import numpy as np

from oracle import cloud_oracle as co
from tests import voxel_ref as vr

VOXEL = 0.01
TVOXEL = 2.0 ** -6
ANCHOR = (-1.0, 2.0, 0.5)


def _attr(n, seed):
    return np.random.default_rng(seed).random((n, 3))


def test_legacy_reference_equals_oracle_and_counts_come_back():
    for shuffle in (True, False):
        p = vr.lattice_cloud(vr.EDGE_COUNTS, VOXEL, 1, ANCHOR, shuffle=shuffle)
        np.testing.assert_array_equal(p[0], ANCHOR)
        np.testing.assert_array_equal(p.min(0), ANCHOR)
        keys, sums, counts = vr.legacy_table(p, VOXEL)
        assert sorted(counts) == sorted(vr.EDGE_COUNTS + [1])
        assert keys[0] == 0 and counts[0] == 1 and (np.diff(keys.astype(np.int64)) > 0).all()
        _, cnt = np.unique(co.voxel_keys(p, VOXEL), axis=0, return_counts=True)
        np.testing.assert_array_equal(cnt, counts)
        col = _attr(len(p), 2)
        want_p, want_c = co.voxel_down_sample(p, VOXEL, colors=col)
        np.testing.assert_array_equal(sums / counts[:, None], want_p)
        np.testing.assert_array_equal(vr.legacy_means(p, p, VOXEL), want_p)
        np.testing.assert_array_equal(vr.legacy_means(col, p, VOXEL), want_c)


def test_tensor_reference_equals_oracle_and_counts_come_back():
    for shuffle in (True, False):
        p = vr.tensor_lattice_cloud(vr.EDGE_COUNTS, TVOXEL, 3, shuffle=shuffle)
        keys, _, counts = vr.tensor_table(p, p, TVOXEL)
        assert sorted(counts) == sorted(vr.EDGE_COUNTS) and keys.min() < 0 < keys.max()
        col = _attr(len(p), 4)
        want_p, want_c = co.voxel_down_sample_tensor(p, TVOXEL, colors=col)
        got_p, got_c = vr.tensor_means(p, p, TVOXEL), vr.tensor_means(col, p, TVOXEL)
        np.testing.assert_array_equal(got_p, want_p)
        np.testing.assert_array_equal(got_c, want_c)
        np.testing.assert_array_equal(got_p, got_p.astype(np.float32).astype(np.float64))


def _order_visible(fwd, rev, counts):
    differs = (fwd != rev).any(1)
    assert not differs[counts <= 2].any()                      # one or two members: addition commutes
    return differs[counts > 192].any() and differs[(counts >= 9) & (counts <= 192)].any()


def test_summation_order_is_visible_in_the_bits():
    p = vr.lattice_cloud(vr.EDGE_COUNTS, VOXEL, 1, ANCHOR)
    _, fwd, counts = vr.legacy_table(p, VOXEL)
    _, rev, _ = vr.legacy_table(p, VOXEL, reverse=True)
    assert _order_visible(fwd, rev, counts)
    col = _attr(len(p), 2)
    assert _order_visible(vr.legacy_table(p, VOXEL, attr=col)[1], vr.legacy_table(p, VOXEL, attr=col, reverse=True)[1], counts)
    t = vr.tensor_lattice_cloud(vr.EDGE_COUNTS, TVOXEL, 3)
    for a in (t, _attr(len(t), 4)):
        _, fwd, counts = vr.tensor_table(a, t, TVOXEL)
        assert fwd.dtype == np.float32
        assert _order_visible(fwd, vr.tensor_table(a, t, TVOXEL, reverse=True)[1], counts)


def test_running_sums_continued_frame_by_frame_equal_the_full_table():
    """the property the resident model's table rests on: with the origin fixed by row 0, a table carried from frame to frame
    (per packed key: the running sum continued member by member, the count) is the full pass's table after every frame"""
    p = vr.lattice_cloud(vr.EDGE_COUNTS, VOXEL, 1, ANCHOR)
    origin = np.asarray(ANCHOR) - VOXEL / 2
    cuts = [0, 400, 1500, 1501, len(p)]
    table = {}
    sizes = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        for k, row in zip(vr.pack_keys(vr.legacy_keys(p[a:b], VOXEL, origin)), p[a:b]):
            s, c = table.get(int(k), (np.zeros(3), 0))
            table[int(k)] = (s + row, c + 1)
        keys, sums, counts = vr.legacy_table(p[:b], VOXEL)
        assert sorted(table) == [int(k) for k in keys]
        np.testing.assert_array_equal(np.stack([table[int(k)][0] for k in keys]), sums)
        np.testing.assert_array_equal([table[int(k)][1] for k in keys], counts)
        sizes.append(len(keys))
    assert sizes[-1] == len(vr.EDGE_COUNTS) + 1 and sizes[0] < sizes[-1]
