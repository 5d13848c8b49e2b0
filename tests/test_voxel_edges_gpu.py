"""The voxel grid entry by entry at the edges of its kernels (csrc/cloud.hip).

Mean kernels (k_voxel_mean_sorted, k_voxel_mean_t, k_voxel_mean_big, double and float): voxels whose member counts sit on the
8-member rounds, the 64-member chunks and VM_BIG = 192; waves of k_voxel_mean_t with every kind of big-voxel mask; more than 4 096
big voxels (the grid-stride loop of _big).  Resident model table (k_vt_build / _update / _merge / _means, model_target_voxels):
every branch driven on purpose and the table read out through r3d_model_debug_voxel_table after every step; error returns injected
through r3d_model_debug_fail_table_step, after which the next call has to rebuild the table of all rows.

A voxel's mean is its members added in index order and the library is built with -ffp-contract=off, so every comparison with
tests/voxel_ref.py is for equality."""
import functools

import numpy as np
import pytest
from numpy.testing import assert_array_equal

from oracle import cloud_oracle as co
from tests import voxel_ref as vr

pytestmark = pytest.mark.gpu
V = 0.01
TV = 2.0 ** -6
ANCHOR = np.array([-1.0, 2.0, 0.5])
CELLS = vr.default_cells(len(vr.EDGE_COUNTS), 1, 1, 13)          # the cells of _base()'s voxels, in list order
BIG = 193                                                        # the smallest voxel k_voxel_mean_big sums


def _attrs(n, seed):
    rng = np.random.default_rng(seed)
    nrm = rng.normal(size=(n, 3))
    return rng.random((n, 3)), nrm / np.linalg.norm(nrm, axis=1, keepdims=True)


@functools.lru_cache(maxsize=None)
def _base():
    p = vr.lattice_cloud(vr.EDGE_COUNTS, V, 1, ANCHOR, cells=CELLS)
    p.setflags(write=False)
    return p


def _check_means(r3d, p, voxel, tensor, col=None, nrm=None):
    """points through k_voxel_mean_sorted, colours / normals through k_voxel_mean_t + _big; returns the number of voxels"""
    got = r3d.cloud_ops.voxel_down_sample(p, voxel, col, nrm, tensor=tensor)
    ref = vr.tensor_means if tensor else vr.legacy_means
    for g, a in zip(got, (p, col, nrm)):
        if a is None:
            assert g is None
            continue
        want = ref(a, p, voxel)
        assert g.shape == want.shape
        assert_array_equal(g, want)
        if tensor:
            assert_array_equal(g, g.astype(np.float32).astype(np.float64))
    return len(got[0])


# ------------------------------------------------------------------------------------------------ mean kernels
@pytest.mark.parametrize("shuffle", [True, False], ids=["shuffled", "contiguous"])
def test_legacy_means_at_edge_counts(r3d, shuffle):
    p = vr.lattice_cloud(vr.EDGE_COUNTS, V, 1, ANCHOR, shuffle=shuffle, cells=CELLS)
    col, nrm = _attrs(len(p), 2)
    assert _check_means(r3d, p, V, False, col, nrm) == len(vr.EDGE_COUNTS) + 1


@pytest.mark.parametrize("shuffle", [True, False], ids=["shuffled", "contiguous"])
def test_tensor_means_at_edge_counts(r3d, shuffle):
    p = vr.tensor_lattice_cloud(vr.EDGE_COUNTS, TV, 3, shuffle=shuffle)
    col, nrm = _attrs(len(p), 4)
    assert _check_means(r3d, p, TV, True, col, nrm) == len(vr.EDGE_COUNTS)


def _wave_masks():
    """320 voxel sizes in key order, 64 per wave of k_voxel_mean_t: no big voxel, one in the first lane, one in the last lane, all
    64, every other lane"""
    s = np.ones((5, 64), np.int64)
    s[1, 0] = s[2, 63] = BIG
    s[3, :] = BIG
    s[4, ::2] = BIG
    return s.reshape(-1)


def _every_fifth(nseg):
    s = np.ones(nseg, np.int64)
    s[4::5] = BIG
    s[-1] = BIG                                                   # the last segment ends at n, not at starts[s + 1]
    return s


SEQUENCES = {"wave_masks": _wave_masks(), "nseg255": _every_fifth(255), "nseg256": _every_fifth(256), "nseg257": _every_fifth(257)}


@pytest.mark.parametrize("tensor", [False, True], ids=["legacy", "tensor"])
@pytest.mark.parametrize("name", list(SEQUENCES))
def test_big_list_shapes(r3d, name, tensor):
    """the voxel sequence in key order is SEQUENCES[name] (thread s of k_voxel_mean_t has voxel s): sizes 1 and 193 only"""
    seq = SEQUENCES[name]
    if tensor:
        p = vr.tensor_lattice_cloud(seq, TV, 5, cells=vr.ordered_cells(len(seq), first=-3))
        assert_array_equal(vr.tensor_table(p, p, TV)[2], seq)
    else:                                                          # segment 0 is the anchor's voxel, of one member like seq[0]
        assert seq[0] == 1
        p = vr.lattice_cloud(seq[1:], V, 5, ANCHOR, cells=vr.ordered_cells(len(seq) - 1))
        assert_array_equal(vr.legacy_table(p, V)[2], seq)
    col, _ = _attrs(len(p), 6)
    assert _check_means(r3d, p, TV if tensor else V, tensor, col) == len(seq)


@pytest.mark.parametrize("tensor", [False, True], ids=["legacy", "tensor"])
def test_single_big_voxel(r3d, tensor):
    """nseg = 1: the only voxel is big, so k_voxel_mean_t writes nothing and one block of k_voxel_mean_big writes everything"""
    rng = np.random.default_rng(7)
    p = (np.array([3, -2, 1]) + 0.1 + 0.4 * rng.random((BIG, 3))) * (TV if tensor else V)
    col, nrm = _attrs(BIG, 8)
    assert _check_means(r3d, p, TV if tensor else V, tensor, col, nrm) == 1


def test_more_big_voxels_than_blocks(r3d):
    """4 100 voxels of 193 members: k_voxel_mean_big is launched with 4 096 blocks, so four of them take a second voxel"""
    p = vr.lattice_cloud([BIG] * 4100, V, 9, ANCHOR, cells=vr.ordered_cells(4100))
    assert len(p) == 791301
    col, _ = _attrs(len(p), 10)
    assert _check_means(r3d, p, V, False, col) == 4101


# ------------------------------------------------------------------------------------------------ resident model table
def _box(rows):
    return np.concatenate([rows.min(0), rows.max(0)])


def _check_table(model, rows, voxel, rebuilds, updates):
    """the table after debug_voxel_table(voxel) against the reference table of all model rows; returns the number of voxels"""
    t = model.debug_voxel_table(voxel)
    keys, sums, counts = vr.legacy_table(rows, voxel)
    assert t["resident"] and t["n"] == len(keys)
    assert_array_equal(t["keys"], keys)
    assert_array_equal(t["counts"], counts)
    assert_array_equal(t["sums"], sums)
    assert_array_equal(t["means"], sums / counts[:, None])
    assert_array_equal(t["means"], co.voxel_down_sample(rows, voxel))
    assert_array_equal(t["box"], _box(rows))
    assert model.voxel_table_stats() == (len(keys), rebuilds, updates)
    return len(keys)


def _check_fallback(model, rows, voxel, rebuilds, updates):
    t = model.debug_voxel_table(voxel)
    assert not t["resident"] and t["keys"] is None and t["sums"] is None and t["counts"] is None
    want = co.voxel_down_sample(rows, voxel)
    assert t["n"] == len(want)
    assert_array_equal(t["means"], want)
    assert_array_equal(t["box"], _box(rows))
    assert model.voxel_table_stats() == (0, rebuilds, updates)


@pytest.fixture
def model(r3d):
    m = r3d.cloud_ops.ResidentModel()
    yield m
    m.close()


def _frame(counts, cells, seed, lo=0.1):
    f = vr.lattice_members(counts, cells, V, seed, ANCHOR, lo)
    return f[np.random.default_rng([seed, 4]).permutation(len(f))]


def test_table_build_at_edge_counts(model):
    model.append(_base())
    assert model.voxel_table_stats() == (0, 0, 0)
    assert _check_table(model, _base(), V, 1, 0) == len(vr.EDGE_COUNTS) + 1
    _check_table(model, _base(), V, 1, 0)                        # nothing appended since: neither a rebuild nor an update


def test_table_update_without_new_voxel(model):
    """frames into existing voxels only, the anchor's included (above the anchor, so the minimum stays): the sums continue in
    place in the buffer that is not swapped, and the second frame reads them there again"""
    rows = _base()
    model.append(rows)
    n = _check_table(model, rows, V, 1, 0)
    rng = np.random.default_rng(11)
    for step in (1, 2):
        f = np.concatenate([_frame(rng.integers(1, 20, len(CELLS)), CELLS, 20 + step), _frame([5], [[0, 0, 0]], 30 + step, lo=0.6)])
        model.append(f)
        rows = np.concatenate([rows, f])
        assert _check_table(model, rows, V, 1, step) == n


def _old_cells_from_3():
    return CELLS + [2, 0, 0]


PLACEMENTS = {
    # old voxels at kx >= 3, new ones at kx in {1, 2}: every new key lies between the anchor's voxel and the smallest other key
    "between": (_old_cells_from_3, lambda: [[1 + i % 2, 1 + i // 4, 1 + i % 5] for i in range(12)]),
    "above": (lambda: CELLS, lambda: [[20 + i // 6, 1 + i % 6, 2] for i in range(12)]),
    "interleaved": (lambda: vr.ordered_cells(48)[0::2], lambda: vr.ordered_cells(48)[1::2]),
}


@pytest.mark.parametrize("placement", list(PLACEMENTS))
def test_table_update_with_only_new_voxels(model, placement):
    old, new = (np.asarray(f()) for f in PLACEMENTS[placement])
    rows = vr.lattice_cloud(vr.EDGE_COUNTS, V, 1, ANCHOR, cells=old)
    model.append(rows)
    n = _check_table(model, rows, V, 1, 0)
    keys_old = vr.legacy_table(rows, V)[0]
    f = _frame(np.random.default_rng(12).integers(1, 30, len(new)), new, 40)
    model.append(f)
    rows = np.concatenate([rows, f])
    assert _check_table(model, rows, V, 1, 1) == n + len(new)
    keys_new = np.setdiff1d(vr.legacy_table(rows, V)[0], keys_old)
    assert len(keys_new) == len(new)
    if placement == "between":
        assert keys_old[0] == 0 and (keys_new > 0).all() and keys_new.max() < keys_old[1]
    elif placement == "above":
        assert keys_new.min() > keys_old.max()
    else:
        merged = np.sort(np.concatenate([keys_old[1:], keys_new]))
        assert np.isin(merged[0::2], keys_old).all() and np.isin(merged[1::2], keys_new).all()


def test_table_mixed_frame_across_blocks(model):
    """more than 256 voxels in the table and more than 256 runs in the frame, continuing runs next to new ones: k_vt_update and
    both branches of k_vt_merge cross a block; then frames of a single point, into an old voxel and into a new one"""
    cells = vr.ordered_cells(700)
    rng = np.random.default_rng(13)
    old = cells[0::2]
    oc = rng.integers(1, 13, len(old))
    oc[::50] = 200
    rows = vr.lattice_cloud(oc, V, 50, ANCHOR, cells=old)
    model.append(rows)
    assert _check_table(model, rows, V, 1, 0) == 351
    sel = cells[np.arange(700) % 3 != 0]
    fc = rng.integers(1, 13, len(sel))
    fc[::40] = 200
    f = _frame(fc, sel, 51)
    model.append(f)
    rows = np.concatenate([rows, f])
    n_new = int((np.flatnonzero(np.arange(700) % 3 != 0) % 2 == 1).sum())
    assert len(sel) > 256 and n_new > 100 and len(sel) - n_new > 100
    assert _check_table(model, rows, V, 1, 1) == 351 + n_new
    for step, cell in ((2, cells[0]), (3, [30, 1, 1])):           # cells[0] is old
        f = _frame([1], [cell], 52 + step)
        model.append(f)
        rows = np.concatenate([rows, f])
        assert _check_table(model, rows, V, 1, step) == 351 + n_new + (step == 3)


def test_table_corners(model):
    """minimum corner equal on every axis: update; below on one axis by a tenth of a voxel: rebuild (every key changes); only the
    maximum corner raised: update, and the box grows"""
    rows = _base()
    model.append(rows)
    _check_table(model, rows, V, 1, 0)
    f = np.concatenate([ANCHOR[None], _frame([3, 4, 5], CELLS[:3], 60)])
    assert_array_equal(f.min(0), rows.min(0))
    model.append(f)
    rows = np.concatenate([rows, f])
    _check_table(model, rows, V, 1, 1)
    for axis in range(3):
        low = rows.min(0).copy()
        low[axis] -= 0.1 * V
        f = np.concatenate([_frame([2, 9], CELLS[3:5], 61 + axis), low[None]])
        assert (f.min(0) < rows.min(0)).tolist() == [a == axis for a in range(3)]
        model.append(f)
        rows = np.concatenate([rows, f])
        _check_table(model, rows, V, 2 + axis, 1)
    f = _frame([6], [[40, 41, 42]], 65)
    assert (f.min(0) > rows.min(0)).all() and (f.max(0) > rows.max(0)).all()
    before = model.debug_voxel_table(V)["box"]
    model.append(f)
    rows = np.concatenate([rows, f])
    _check_table(model, rows, V, 4, 2)
    after = model.debug_voxel_table(V)["box"]
    assert_array_equal(after[:3], before[:3])
    assert (after[3:] > before[3:]).all()


def test_table_voxel_size_change_rebuilds(model):
    model.append(_base())
    for k, voxel in enumerate((0.01, 0.02, 0.01)):
        _check_table(model, _base(), voxel, k + 1, 0)


def test_table_after_clear(model):
    """the table describes the new rows only, for a new model shorter and one longer than the rows the old table covered"""
    model.append(_base())
    _check_table(model, _base(), V, 1, 0)
    short = vr.lattice_cloud([3, 9, 200], V, 70, (0.25, -3.0, 1.0))
    longer = vr.lattice_cloud(vr.EDGE_COUNTS + [500, 17], V, 71, (5.0, 5.0, -5.0))
    assert len(short) < len(_base()) < len(longer)
    for k, rows in enumerate((short, longer)):
        model.clear()
        assert model.voxel_table_stats() == (0, 1 + k, 0) and len(model) == 0
        model.append(rows)
        _check_table(model, rows, V, 2 + k, 0)
    f = _frame([4, 4], [[2, 2, 2], [50, 1, 1]], 72, ) + (np.array([5.0, 5.0, -5.0]) - ANCHOR)
    model.append(f)                                               # and the table of the new model goes on incrementally
    _check_table(model, np.concatenate([longer, f]), V, 3, 1)


def test_table_key_space_fallback(model):
    """more than 2^21 voxels along an axis: no table, the plain full pass -- reached from a rebuild and from an update"""
    far = np.array([[0.0, 0.0, 0.0], [30.0, 0.0, 0.0]])
    model.append(far)
    _check_fallback(model, far, 1e-5, 0, 0)
    model.clear()
    rows = _base()
    model.append(rows)
    _check_table(model, rows, V, 1, 0)
    f = _frame([3, 1], [CELLS[0], [2_200_000, 3, 3]], 80)         # raises the maximum on x beyond 2^21 voxels from the origin
    model.append(f)
    rows = np.concatenate([rows, f])
    _check_fallback(model, rows, V, 1, 0)
    _check_fallback(model, rows, V, 1, 0)                        # and stays without a table
    model.clear()
    small = vr.lattice_cloud([2, 10], V, 81, ANCHOR)
    model.append(small)
    _check_table(model, small, V, 2, 0)


def test_table_refusals(r3d, model):
    with pytest.raises(r3d.R3DError):
        model.debug_voxel_table(V)                               # empty model
    model.append(_base())
    for bad in (0.0, -0.01, float("nan")):
        with pytest.raises(r3d.R3DError):
            model.debug_voxel_table(bad)
    assert model.voxel_table_stats() == (0, 0, 0)
    t = model.debug_voxel_table(V, cap=len(vr.EDGE_COUNTS))      # one short
    assert t["n"] == len(vr.EDGE_COUNTS) + 1 and t["resident"]
    assert all(t[k] is None for k in ("keys", "sums", "counts", "means", "box"))
    assert model.voxel_table_stats() == (t["n"], 1, 0)           # the table was built all the same
    assert model.debug_voxel_table(V, cap=t["n"])["keys"].shape == (t["n"],)
    _check_table(model, _base(), V, 1, 0)


def test_table_after_align_append(model):
    """the public path: align_append updates the table itself and appends the aligned frame (whose bounding box is computed on the
    device for the next call, pend_lo / pend_hi); a plain append in between makes the next update cover both blocks"""
    model.append(_base())
    n0 = len(_base())
    src = _base()[1::3]                                           # the model's own points: the aligned frame stays inside the box
    res = model.align_append(src, threshold=0.02, voxel_size=V, max_iteration=1)
    assert res["appended"] > 0 and model.voxel_table_stats() == (len(vr.EDGE_COUNTS) + 1, 1, 0)
    rows = model.download()[0]
    assert_array_equal(rows[:n0], _base())
    assert len(rows) == n0 + res["appended"] and (rows[n0:].min(0) >= rows[:n0].min(0)).all()
    _check_table(model, rows, V, 1, 1)
    res2 = model.align_append(_base()[2::3], threshold=0.02, voxel_size=V, max_iteration=1)
    assert model.voxel_table_stats()[1:] == (1, 1)               # the table was up to date: nothing to do
    f = _frame([2, 2, 7], [CELLS[5], [9, 14, 3], [1, 1, 14]], 90)
    model.append(f)
    rows = model.download()[0]
    assert len(rows) == n0 + res["appended"] + res2["appended"] + len(f) and (rows[n0:].min(0) >= rows[:n0].min(0)).all()
    assert_array_equal(rows[-len(f):], f)
    _check_table(model, rows, V, 1, 2)


# ------------------------------------------------------------------------------------------------ error returns
# r3d_model_debug_fail_table_step injects the error return only (no launch changes), at 1: a rebuild after k_vt_build, 2: an update
# after k_vt_update has added the slice to the resident sums, 3: an update after k_vt_merge.  Whatever stops a call, the table is
# marked valid only after its last fallible step, so the next call rebuilds from the model's rows.
def _old_voxel_frames():
    """the two frames of test_table_update_without_new_voxel: existing voxels only, so no k_vt_merge"""
    rng = np.random.default_rng(11)
    return [np.concatenate([_frame(rng.integers(1, 20, len(CELLS)), CELLS, 20 + step), _frame([5], [[0, 0, 0]], 30 + step, lo=0.6)])
            for step in (1, 2)]


def _mixed_frame():
    """the first of those frames and the twelve new cells of the "above" placement: k_vt_merge runs"""
    new = np.asarray(PLACEMENTS["above"][1]())
    return np.concatenate([_old_voxel_frames()[0], _frame(np.random.default_rng(12).integers(1, 30, len(new)), new, 40)])


FAIL_FRAMES = {"F_old": lambda: _old_voxel_frames()[0], "F_mix": _mixed_frame}


@pytest.mark.parametrize("step,frame", [(2, "F_old"), (2, "F_mix"), (3, "F_mix")])
def test_table_failed_update_forces_rebuild(r3d, model, step, frame):
    """an update that returns an error after k_vt_update (the slice is in the resident sums already) or after k_vt_merge leaves no
    table; the next call rebuilds it from all rows -- sums equal to the reference's, so the slice was not added twice -- and the
    incremental path goes on from there"""
    rows = _base()
    model.append(rows)
    _check_table(model, rows, V, 1, 0)
    f = FAIL_FRAMES[frame]()
    assert (f.min(0) >= rows.min(0)).all()                       # the minimum corner stays: an update, not a rebuild
    model.append(f)
    rows = np.concatenate([rows, f])
    model.debug_fail_table_step(step)
    with pytest.raises(r3d.R3DError, match="injected"):
        model.debug_voxel_table(V)
    assert model.voxel_table_stats() == (0, 1, 0)
    _check_table(model, rows, V, 2, 0)
    f2 = _old_voxel_frames()[1]
    model.append(f2)
    _check_table(model, np.concatenate([rows, f2]), V, 2, 1)


def test_table_failed_rebuild_leaves_no_table(r3d, model):
    """a rebuild for another voxel size that returns an error after k_vt_build has overwritten the buffers: no table, not the new
    one under the old label; and the same for the first build of a model"""
    model.append(_base())
    n = _check_table(model, _base(), V, 1, 0)
    assert model.voxel_table_stats() == (n, 1, 0)
    model.debug_fail_table_step(1)
    with pytest.raises(r3d.R3DError, match="injected"):
        model.debug_voxel_table(0.02)
    assert model.voxel_table_stats() == (0, 1, 0)
    _check_table(model, _base(), V, 2, 0)
    fresh = r3d.cloud_ops.ResidentModel()
    try:
        fresh.append(_base())
        fresh.debug_fail_table_step(1)
        with pytest.raises(r3d.R3DError, match="injected"):
            fresh.debug_voxel_table(V)
        assert fresh.voxel_table_stats() == (0, 0, 0)
        _check_table(fresh, _base(), V, 1, 0)
    finally:
        fresh.close()


def test_align_append_after_failed_update_equals_undisturbed(r3d):
    """the public path: an align_append whose table update returns an error changes no row of the model, and the next one (which
    rebuilds) gives bit for bit what a model that never saw the error gives (which updates)"""
    a, b = r3d.cloud_ops.ResidentModel(), r3d.cloud_ops.ResidentModel()
    try:
        rows = np.concatenate([_base(), _mixed_frame()])
        for m in (a, b):
            m.append(_base())
            _check_table(m, _base(), V, 1, 0)
            m.append(_mixed_frame())
        src = _base()[1::3]
        a.debug_fail_table_step(2)
        with pytest.raises(r3d.R3DError, match="injected"):
            a.align_append(src, threshold=0.02, voxel_size=V, max_iteration=1)
        assert len(a) == len(rows)
        got = a.download()
        assert_array_equal(got[0], rows)
        assert got[1] is None and got[2] is None
        ra, rb = (m.align_append(src, threshold=0.02, voxel_size=V, max_iteration=1) for m in (a, b))
        assert_array_equal(ra["T"], rb["T"])
        for k in ("fitness", "inlier_rmse", "iterations", "correspondences", "appended"):
            assert ra[k] == rb[k], k
        assert ra["appended"] > 0
        da, db = a.download(), b.download()
        assert_array_equal(da[0], db[0])
        assert_array_equal(da[0][:len(rows)], rows)
        for x, y in zip(da[1:], db[1:]):
            assert (x is None and y is None) or np.array_equal(x, y)
        n = len(vr.legacy_table(rows, V)[0])                      # the table covers the rows the frame was aligned to
        assert a.voxel_table_stats() == (n, 2, 0) and b.voxel_table_stats() == (n, 1, 1)
    finally:
        a.close()
        b.close()


def test_fail_hook_arming(r3d, model):
    """steps outside 0..3 are refused; the hook is cleared when the next table call starts, whether or not that call reaches the
    step; step 0 disarms"""
    for bad in (-1, 4):
        with pytest.raises(r3d.R3DError):
            model.debug_fail_table_step(bad)
    rows = _base()
    model.append(rows)
    _check_table(model, rows, V, 1, 0)
    f1, f2 = _old_voxel_frames()
    new = np.asarray(PLACEMENTS["above"][1]())
    for k, (arm, f) in enumerate((((3,), f1),                      # no merge in this update: step 3 is never reached
                                  ((), _frame([3] * len(new), new, 41)),   # a merge: step 3 would fire here, were it still armed
                                  ((2, 0), f2))):                # disarmed again before the call
        for s in arm:
            model.debug_fail_table_step(s)
        model.append(f)
        rows = np.concatenate([rows, f])
        _check_table(model, rows, V, 1, k + 1)
