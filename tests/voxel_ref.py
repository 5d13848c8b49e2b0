"""References for the voxel grids of csrc/cloud.hip (k_voxel_mean_sorted / _t / _big and the resident model's table, k_vt_*) and
the deterministic clouds they are tested on.  Plain numpy, no GPU.

A voxel's sum is its members added ONE AT A TIME IN INDEX ORDER, in the grid's own precision (float64 legacy, float32 tensor);
the library is built with -ffp-contract=off and its kernels keep that order, so every comparison against these functions is for
EQUALITY.  The sums are formed by an explicit sequential scheme (round r adds member r of every voxel that has one, the loop of
oracle.cloud_oracle.voxel_down_sample_tensor) -- never np.sum or np.add.reduceat, which add pairwise."""
import numpy as np

# member counts around the kernels' boundaries: the 8-member rounds of k_voxel_mean_sorted / _t / k_vt_build, the 64-member
# chunks of k_voxel_mean_big and VM_BIG = 192 (larger voxels are listed by _t and summed by _big)
EDGE_COUNTS = [1, 2, 7, 8, 9, 15, 16, 17, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 319, 320, 321, 449]
KEY_BITS = 21


def pack_keys(k):
    """kx << 42 | ky << 21 | kz of int64 [n,3] voxel indices in [0, 2^21)"""
    k = np.asarray(k, np.int64).reshape(-1, 3)
    assert k.size == 0 or (k.min() >= 0 and k.max() < 1 << KEY_BITS)
    u = k.astype(np.uint64)
    return u[:, 0] << np.uint64(2 * KEY_BITS) | u[:, 1] << np.uint64(KEY_BITS) | u[:, 2]


def _segments(keys3):
    """(order, starts, counts, unique keys): the stable sort of the rows by (kx, ky, kz) and its runs of equal key"""
    order = np.lexsort((keys3[:, 2], keys3[:, 1], keys3[:, 0]))          # lexsort is stable: members stay in index order
    ks = keys3[order]
    first = np.concatenate([[True], (ks[1:] != ks[:-1]).any(1)])
    starts = np.flatnonzero(first)
    counts = np.diff(np.concatenate([starts, [len(ks)]]))
    return order, starts, counts, ks[starts]


def _sequential_sums(a_sorted, starts, counts, dtype, reverse=False):
    """[nvox,3] sums in `dtype`: round r adds member r (reverse: member count-1-r) of every voxel that still has one"""
    a = np.asarray(a_sorted, dtype)
    out = np.zeros((len(starts), 3), dtype)
    pos = np.zeros(len(starts), np.int64)
    live = np.arange(len(starts))
    while live.size:
        at = starts[live] + (counts[live] - 1 - pos[live] if reverse else pos[live])
        out[live] = out[live] + a[at]
        pos[live] += 1
        live = live[pos[live] < counts[live]]
    return out


def legacy_keys(points, voxel, origin=None):
    p = np.asarray(points, np.float64).reshape(-1, 3)
    origin = p.min(0) - voxel / 2 if origin is None else np.asarray(origin, np.float64)
    return np.floor((p - origin) / voxel).astype(np.int64)


def legacy_table(points, voxel, origin=None, attr=None, reverse=False):
    """(packed keys uint64 [n], sums float64 [n,3], counts int32 [n]) of the legacy grid (origin = min - voxel / 2 unless given), in
    ascending (kx, ky, kz) order; the sums are those of `attr` (default: the points themselves)"""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    order, starts, counts, keys = _segments(legacy_keys(p, voxel, origin))
    a = p if attr is None else np.asarray(attr, np.float64).reshape(-1, 3)
    return pack_keys(keys), _sequential_sums(a[order], starts, counts, np.float64, reverse), counts.astype(np.int32)


def legacy_means(attr, points, voxel):
    """per-voxel means of an [n,3] attribute over the legacy grid of `points` (VoxelDownSample: float64 sum / float64 count)"""
    _, sums, counts = legacy_table(points, voxel, attr=attr)
    return sums / counts.astype(np.float64)[:, None]


def tensor_table(attr, points, voxel, reverse=False):
    """(keys int64 [n,3], sums float32 [n,3], counts int32 [n]) of the tensor grid: inputs rounded to float32, key =
    floor(float32(p) / float32(voxel)) from origin 0, float32 sums; ascending (kx, ky, kz) order"""
    p32 = np.asarray(points, np.float64).reshape(-1, 3).astype(np.float32)
    keys3 = np.floor(p32 / np.float32(voxel)).astype(np.int64)
    order, starts, counts, keys = _segments(keys3)
    a32 = np.asarray(attr, np.float64).reshape(-1, 3).astype(np.float32)
    return keys, _sequential_sums(a32[order], starts, counts, np.float32, reverse), counts.astype(np.int32)


def tensor_means(attr, points, voxel):
    """per-voxel means of the tensor method: float32 sum / float32 count, returned as float64 holding float32 values"""
    _, sums, counts = tensor_table(attr, points, voxel)
    return (sums / counts.astype(np.float32)[:, None]).astype(np.float64)


def default_cells(n, seed, lo, hi):
    """n distinct integer cells with every index in [lo, hi), in a seeded random order"""
    side = hi - lo
    assert side ** 3 >= n
    flat = np.random.default_rng([seed, 1]).permutation(side ** 3)[:n]
    return np.stack([flat // (side * side), flat // side % side, flat % side], 1) + lo


def _members(counts, cells, seed, lo=0.1):
    """cell-relative member positions (cell + lo + (0.9 - lo) * random, strictly inside the cell) of all voxels, voxel after voxel"""
    counts = np.asarray(counts, np.int64)
    cells = np.asarray(cells, np.int64).reshape(-1, 3)
    assert len(cells) == len(counts) and len(np.unique(cells, axis=0)) == len(cells), "cells must be distinct, one per voxel"
    rng = np.random.default_rng([seed, 2])
    return np.repeat(cells, counts, axis=0) + lo + (0.9 - lo) * rng.random((int(counts.sum()), 3))


def _shuffled(rows, seed, keep_first):
    perm = np.random.default_rng([seed, 3]).permutation(len(rows) - keep_first) + keep_first
    return rows[np.concatenate([np.arange(keep_first), perm])]


def lattice_members(counts, cells, voxel, seed, anchor=(-1.0, 2.0, 0.5), lo=0.1):
    """counts[i] members in cell cells[i] of the grid whose origin is anchor - voxel / 2 (no anchor row), voxel after voxel: a
    frame for a model that lattice_cloud started.  lo = 0.6 keeps members of cell (0, 0, 0) above the anchor on every axis."""
    return (np.asarray(anchor, np.float64) - voxel / 2) + _members(counts, cells, seed, lo) * voxel


def lattice_cloud(counts, voxel, seed, anchor=(-1.0, 2.0, 0.5), shuffle=True, cells=None):
    """A cloud for the LEGACY grid: row 0 is `anchor`, the minimum on every axis, so the grid's origin is anchor - voxel / 2 and the
    anchor sits alone in voxel (0, 0, 0).  Voxel i of the list gets counts[i] members in cell cells[i] (distinct, every index
    >= 1 -- a member sharing an index 0 with the anchor could lie below it and move the origin; default: default_cells in
    [1, 13)^3), each strictly inside the cell at (0.1 + 0.8 * random) of the voxel from the cell's corner, so that no key depends on
    a rounding.  shuffle: the rows after the anchor are permuted, a voxel's members are then scattered through the index range;
    otherwise they are contiguous, voxel after voxel in list order.  The grid has len(counts) + 1 voxels."""
    anchor = np.asarray(anchor, np.float64)
    cells = default_cells(len(counts), seed, 1, 13) if cells is None else np.asarray(cells, np.int64).reshape(-1, 3)
    assert cells.min() >= 1
    rows = np.concatenate([anchor[None], lattice_members(counts, cells, voxel, seed, anchor)])
    return _shuffled(rows, seed, 1) if shuffle else rows


def tensor_lattice_cloud(counts, voxel, seed, shuffle=True, cells=None):
    """The same for the TENSOR grid (origin 0, no anchor): voxel is a power of two, cells are integer multiples of it (default:
    default_cells in [-6, 6)^3, so some indices are negative), members at (cell + 0.1 + 0.8 * random) * voxel -- the float32
    rounding of the inputs moves a member by 1e-6 of a cell at most.  The grid has len(counts) voxels."""
    assert np.log2(voxel) == np.round(np.log2(voxel))
    cells = default_cells(len(counts), seed, -6, 6) if cells is None else cells
    rows = _members(counts, cells, seed) * voxel
    return _shuffled(rows, seed, 0) if shuffle else rows


def ordered_cells(n, first=1):
    """n cells in ascending (kx, ky, kz) order, every index >= first: voxel i of a lattice cloud is then the i-th in key order"""
    i = np.arange(n)
    return np.stack([i // 64, i // 8 % 8, i % 8], 1) + first
