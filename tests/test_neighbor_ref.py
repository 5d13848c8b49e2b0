"""CPU checks of tests/neighbor_ref.py: the brute-force reference agrees with a kd-tree where a kd-tree can be trusted, the
oracle's kd-tree helper cannot referee tie-heavy clouds (why the reference exists), and the clouds have the properties the GPU
tests (tests/test_neighbor_search_gpu.py) rely on."""
import numpy as np
import pytest
from scipy.spatial import cKDTree

from oracle import cloud_oracle as co
from tests import neighbor_ref as nr


def test_reference_equals_kdtree_on_a_generic_cloud():
    rng = np.random.default_rng(1)
    p, q = rng.random((900, 3)), rng.random((300, 3)) * 1.2 - 0.1
    tree = cKDTree(p)
    idx, d2 = nr.brute_knn(p, q, 9)
    d, i = tree.query(q, k=9)
    np.testing.assert_array_equal(idx, i)                       # no ties in a random float64 cloud
    assert np.abs(np.sqrt(d2) - d).max() < 1e-15
    r = 0.11
    ri, rd2 = nr.brute_knn(p, q, 9, radius=r)
    d, i = tree.query(q, k=9, distance_upper_bound=r)
    np.testing.assert_array_equal(ri, np.where(np.isinf(d), -1, i))
    assert ((rd2 == nr.PAD_D2) == np.isinf(d)).all() and (ri >= 0).any() and (ri < 0).any()
    np.testing.assert_array_equal(nr.brute_count(p, r), tree.query_ball_point(p, r, return_length=True))
    T = np.eye(4)
    T[:3, :3] = [[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]
    T[:3, 3] = [1.0, 0.0, 0.02]
    corr, nd2 = nr.brute_nearest(p, q, T, 0.05)
    d, i = tree.query(nr.transform(T, q), k=1, distance_upper_bound=0.05)
    np.testing.assert_array_equal(corr, np.where(np.isinf(d), -1, i))
    hit = corr >= 0
    assert hit.any() and (~hit).any() and np.abs(np.sqrt(nd2[hit]) - d[hit]).max() < 1e-15 and (nd2[~hit] == nr.PAD_D2).all()


def test_restrict_is_brute_knn_with_smaller_k_and_a_radius():
    p = nr.cases()["lattice"]
    full = nr.reference_lists("lattice")
    for k, r in ((1, None), (16, nr.LATTICE_H), (40, 2 * nr.LATTICE_H), (40, None)):
        a, b = nr.restrict(*full, k, r), nr.brute_knn(p, p, k, r)
        np.testing.assert_array_equal(a[0], b[0])
        np.testing.assert_array_equal(a[1], b[1])


def test_kdtree_helper_of_the_oracle_cannot_referee_the_lattice():
    """_nearest_total_order re-orders k + 12 kd-tree candidates; at k = 40 the lattice's tie shell at sqrt(5) spacings holds 24
    points, so the helper's lists are an arbitrary choice among them: same distances, other indices."""
    p = nr.cases()["lattice"]
    idx, d2 = nr.restrict(*nr.reference_lists("lattice"), 40)
    hi, hd2 = co._nearest_total_order(p, p, 40)
    np.testing.assert_array_equal(hd2, d2)
    rows = (hi != idx).any(1).sum()
    assert rows > 100, rows
    # the shell: interior points have 24 neighbours at exactly 5 h^2, more than the helper's 12 spare candidates
    full = nr.reference_lists("lattice")[1]
    assert ((full == 5 * nr.LATTICE_H ** 2).sum(1) == 24).any()


def test_clouds_have_the_properties_the_gpu_tests_rely_on():
    c = nr.cases()
    assert list(c) == ["lattice", "surface_patch", "volume_cluster", "far_blobs", "line", "plane", "offset", "tiny"]
    assert all(len(p) <= 4500 and p.dtype == np.float64 for p in c.values())
    # lattice: exact coordinates, distances exactly equal to both radii, index order unrelated to position
    lat = c["lattice"]
    assert len(lat) == 12 ** 3 and (lat / nr.LATTICE_H == np.round(lat / nr.LATTICE_H)).all()
    d2 = nr.reference_lists("lattice")[1]
    assert (d2 == nr.LATTICE_H ** 2).any() and (d2 == (2 * nr.LATTICE_H) ** 2).any()
    assert not (np.lexsort(lat.T[::-1]) == np.arange(len(lat))).all()
    assert nr.knn_radii("lattice") == (0.0, 2.0 ** -7, 2.0 ** -6) and nr.nn_max_dists("lattice") == (2.0 ** -6, 2.0 ** -4)
    # surface_patch / volume_cluster: a 27-cell block of the 1-NN grid (cell <= max_dist) can hold more than 1 024 candidates,
    # beside points that have that ball to themselves
    for name, r in (("surface_patch", 0.5 * nr.spacing("surface_patch")), ("volume_cluster", 15 * nr.spacing("volume_cluster"))):
        cnt = nr.brute_count(c[name], r)
        assert cnt.max() > 1024 and (cnt == 1).sum() > 100, (name, cnt.max(), (cnt == 1).sum())
    # far_blobs: 2 000 m apart; at k = 64 every point of the small blob takes exactly 24 neighbours from the far one
    fb = c["far_blobs"]
    small = np.linalg.norm(fb, axis=1) < 1.0
    assert small.sum() == 40 and abs(np.linalg.norm(fb[~small].mean(0) - fb[small].mean(0)) - 2000.0) < 0.1
    i64 = nr.restrict(*nr.reference_lists("far_blobs"), 64)[0]
    assert ((~small[i64[small]]).sum(1) == 24).all()
    assert 64 in nr.knn_ks("far_blobs") and nr.nn_max_dists("far_blobs") == (1e-3,)
    # line / plane: zero extent along two axes / one axis
    assert (np.ptp(c["line"], axis=0)[1:] == 0).all() and np.ptp(c["line"], axis=0)[0] > 0.9 and len(c["line"]) == 500
    assert np.ptp(c["plane"], axis=0)[2] == 0 and (np.ptp(c["plane"], axis=0)[:2] > 0.9).all() and len(c["plane"]) == 1500
    # offset: surface_patch moved to coordinates around 1e5
    assert np.abs(c["offset"]).min(0).tolist() > [9e4, 1.9e5, 2.9e4]
    a, = (np.sort(np.linalg.norm(c["offset"] - nr.OFFSET, axis=1)),)
    assert np.abs(a - np.sort(np.linalg.norm(c["surface_patch"], axis=1))).max() < 1e-10
    # tiny: k >= n
    assert len(c["tiny"]) == 5 and nr.knn_ks("tiny") == (1, 2, 3, 5)
    assert len(nr.knn_table()) == sum(len(nr.knn_ks(n)) * len(nr.knn_radii(n)) for n in c)


def test_one_nn_sources_cover_the_edges():
    tab = nr.nn_table()
    assert len(tab) == 2 * sum(len(nr.nn_max_dists(n)) for n in nr.cases())
    for cid, name, src, T, md, nothing in tab:
        if T is not None:
            continue
        t = nr.cases()[name]
        corr, d2 = nr.nn_reference(cid)
        n_own = min(nr.NN_OWN, len(t))
        np.testing.assert_array_equal(d2[:n_own], 0.0)           # the target's own points: d = 0 ...
        first = np.array([np.flatnonzero((t == q).all(1))[0] for q in src[:n_own]])
        np.testing.assert_array_equal(corr[:n_own], first)       # ... found at the lowest index that holds them
        lo, hi = t.min(0), t.max(0)
        beyond = np.maximum(np.maximum(lo - src, src - hi), 0).max(1)
        assert (beyond > 30 * md).any() and ((beyond > 0) & (beyond < md)).any() and ((beyond > md) & (beyond < 2 * md)).any()
        assert ((beyond > 0) & (corr >= 0)).any() and ((beyond > 0) & (corr < 0)).any(), cid
        if name == "lattice":
            moved = src[nothing]
            assert len(moved) == 2 * 144 and (corr[nothing] == -1).all() and (d2[nothing] == nr.PAD_D2).all()
            true = nr._pair_d2(t, moved).min(1)
            np.testing.assert_array_equal(true, md * md)         # exactly AT the distance: the strict < drops them
            # tied queries: eight targets at exactly 3/4 h^2 from a cell centre, four at exactly 6.75 h^2 outside an x face;
            # the reference keeps the lowest index
            D = nr._pair_d2(t, src[nothing.stop:])
            ties = (D == D.min(1, keepdims=True)).sum(1)
            assert len(D) == 11 ** 3 + 2 * 121 and (ties[:11 ** 3] == 8).all() and (ties[11 ** 3:] == 4).all()
            h2 = nr.LATTICE_H ** 2
            assert (D.min(1)[:11 ** 3] == 0.75 * h2).all() and (D.min(1)[11 ** 3:] == 6.75 * h2).all()
            want = np.where(D.min(1) < md * md, (D == D.min(1, keepdims=True)).argmax(1), -1)
            np.testing.assert_array_equal(corr[nothing.stop:], want)
            assert (want[11 ** 3:] >= 0).all() == (md > 3 * nr.LATTICE_H)
    # far_blobs at 1e-3: the grid is coarsened to a cell of metres (extent^3 / 2^26 cells), far above the distance
    ext = np.ptp(nr.cases()["far_blobs"], axis=0)
    assert (np.prod(ext) / 2 ** 26) ** (1 / 3) > 1000 * 1e-3


def test_far_lattice_is_beyond_the_packed_search_and_its_reference_is_well_defined():
    """the translated lattice of tests/test_neighbor_search_gpu.py: on the float64 side of the registration's search choice at
    both distances, every coordinate exact, and the tied queries tied in the reference too"""
    from tests import test_neighbor_search_gpu as ts
    t = ts.far_lattice()
    np.testing.assert_array_equal(t - ts.FAR_SHIFT, nr.cases()["lattice"])        # the translation rounded nothing
    assert 1500 < len(t) < 2000
    for cid, src, T, md, nothing, (corr, d2) in ts.far_nn_table():
        # the search grid's cell never exceeds max_dist, so max|coordinate| / cell is at least this
        assert np.abs(t).max() / md >= 1e9, cid
        assert 3000 < len(src) < 6000
        if T is not None:
            continue
        moved = src[nothing]
        assert len(moved) == 2 * 144 and (corr[nothing] == -1).all()
        np.testing.assert_array_equal(nr._pair_d2(t, moved).min(1), md * md)       # exactly AT the distance
        D = nr._pair_d2(t, src[nothing.stop:])
        ties = (D == D.min(1, keepdims=True)).sum(1)
        assert len(D) == 11 ** 3 + 2 * 121 and (ties[:11 ** 3] == 8).all() and (ties[11 ** 3:] == 4).all()
        h2 = nr.LATTICE_H ** 2
        assert (D.min(1)[:11 ** 3] == 0.75 * h2).all() and (D.min(1)[11 ** 3:] == 6.75 * h2).all()
        want = np.where(D.min(1) < md * md, (D == D.min(1, keepdims=True)).argmax(1), -1)
        np.testing.assert_array_equal(corr[nothing.stop:], want)                   # the lowest index among the tied


@pytest.mark.parametrize("name", nr.NORMAL_CLOUDS)
def test_normal_neighbourhoods_are_sheets(name):
    """the well-separated-eigenvector filter of the normal comparison may drop at most 2 % of the points"""
    for k in nr.NORMAL_KS + (20,):
        for radius in nr.NORMAL_RADII:
            normals, comparable, short = nr.normal_reference(name, k, radius)
            excluded = ~comparable & ~short
            assert excluded.mean() <= 0.02, (name, k, radius, excluded.sum())
            assert (normals[short] == [0.0, 0.0, 1.0]).all()
            assert comparable.sum() > 1500                       # the dense patch (1 500 points) and more
    assert nr.normal_reference("surface_patch", 20, None)[1].all()
