"""GPU tests of the stages either side of the matcher (csrc/prepost.hip) at the edges of their kernels: the block structure
of the partitioned WLS solver, every instantiation of the discontinuity map, parameter and ROI variants, the grid-stride and
unaligned paths of normalize, strides / block widths / tiny sources of remap, and the variants of the rectification maps.
Cases, inputs, references and the derivation of the one tolerance are in tests/prepost_cases.py; integer and fixed-point
stages, the confidence map and the sequential solver are compared bit for bit."""
import ctypes

import numpy as np
import pytest

from tests import prepost_cases as pc

pytestmark = pytest.mark.gpu

_vp = ctypes.c_void_p


def _po():
    from oracle import prepost_oracle as po
    return po


def _p(a):
    return a.ctypes.data_as(_vp)


def _params(r3d, c, solver):
    return r3d.stereo_prepost.WlsParams(c.lam, c.sigma, c.att, 0.001, c.min_disp, c.num_disp, c.radius, c.lrc, c.num_iter, solver)


_RUNS = {}


def _run(r3d, c):
    """-> {solver: (out, conf)} of one case through r3d_wls_filter, run once per session."""
    if c not in _RUNS:
        sp = r3d.stereo_prepost
        ref = pc.reference(c)
        gbuf, gstride = pc.padded_guide(c, ref.guide)
        dl, dr = np.ascontiguousarray(ref.dl), np.ascontiguousarray(ref.dr)
        res = {}
        for solver in (sp.SOLVER_PARTITIONED, sp.SOLVER_SEQUENTIAL):
            out = np.full((c.H, c.W), 12345, np.int16)
            conf = np.full((c.H, c.W), np.nan, np.float32)
            p = _params(r3d, c, solver)
            r3d.default_context().call("r3d_wls_filter", ctypes.byref(p), _p(dl), _p(dr), _p(gbuf), c.guide_cn, gstride, c.W, c.H,
                                       _p(out), _p(conf))
            res[solver] = (out, conf)
        _RUNS[c] = res
    return _RUNS[c]


def _where(c, mask):
    """Positions of differing pixels relative to the solver's structure, for the failure message."""
    ys, xs = np.nonzero(mask)
    return [(int(x), int(y), f"x%32={x % 32}", f"y%32={y % 32}", f"tile={y // 64},{x // 64}") for y, x in zip(ys[:12], xs[:12])]


def _check_case(r3d, c):
    sp = r3d.stereo_prepost
    ref = pc.reference(c)
    lx, lw = c.roi()
    res = _run(r3d, c)
    fill = 16 * (c.min_disp - 1)
    for solver, (out, conf) in res.items():
        np.testing.assert_array_equal(conf, ref.conf, err_msg=f"confidence, solver {solver}")
        assert (out[:, :lx] == fill).all() and (out[:, lx + lw:] == fill).all()
        assert not conf[:, :lx].any() and not conf[:, lx + lw:].any()
    np.testing.assert_array_equal(res[sp.SOLVER_SEQUENTIAL][0], ref.want)
    got = res[sp.SOLVER_PARTITIONED][0][:, lx:lx + lw].astype(int)
    diff = np.abs(got - ref.want[:, lx:lx + lw].astype(int))
    print(f"{c.id}: e={ref.e:.3g} tau={ref.tau:.3g} ambiguous={int(ref.ambiguous.sum())}/{diff.size} differ={int((diff > 0).sum())}")
    assert diff.max(initial=0) <= 1, _where(c, diff > 1)
    bad = (diff > 0) & ~ref.ambiguous
    assert not bad.any(), (f"differs where q64 is not within tau={ref.tau:.3g} of a half-integer", _where(c, bad),
                           pc.half_integer_distance(ref.q64[bad])[:12])
    return int((diff > 0).sum()), diff.size


def _ids(cases):
    return [c.id for c in cases]


@pytest.mark.parametrize("c", pc.SOLVER, ids=_ids(pc.SOLVER))
def test_wls_solver_geometry(r3d, c):
    _check_case(r3d, c)


@pytest.mark.parametrize("c", pc.PARAMS, ids=_ids(pc.PARAMS))
def test_wls_parameters(r3d, c):
    _check_case(r3d, c)


@pytest.mark.parametrize("c", pc.DD, ids=_ids(pc.DD))
def test_wls_discontinuity_radius(r3d, c):
    _check_case(r3d, c)


@pytest.mark.parametrize("c", pc.ROI, ids=_ids(pc.ROI))
def test_wls_roi_placement(r3d, c):
    _check_case(r3d, c)
    lx, lw = c.roi()
    if lw == 0:
        for out, conf in _run(r3d, c).values():
            assert (out == 16 * (c.min_disp - 1)).all() and not conf.any()


@pytest.mark.parametrize("table", list(pc.TABLES))
def test_wls_partitioned_pooled_share(r3d, table):
    """include/r3d.h: fewer than 0.1 % of the pixels differ from the sequential order; pooled over a table, since one pixel of
    a 99-pixel case is 1 %."""
    differ = total = 0
    for c in pc.TABLES[table]:
        d, n = _check_case(r3d, c)
        differ += d
        total += n
    print(f"{table}: {differ} of {total} pixels differ")
    assert differ < pc.POOLED_SHARE * total


def test_wls_filter_dev_equals_host_entry(r3d):
    c = pc.SOLVER[-1]                                             # 97 x 64
    sp = r3d.stereo_prepost
    ctx = r3d.default_context()
    ref = pc.reference(c)
    ptrs = [ctx.to_device(ref.dl), ctx.to_device(ref.dr), ctx.to_device(ref.guide), ctx.alloc(c.W * c.H * 2), ctx.alloc(c.W * c.H * 4)]
    try:
        for solver, (want, wconf) in _run(r3d, c).items():
            p = _params(r3d, c, solver)
            out = np.empty((c.H, c.W), np.int16)
            conf = np.empty((c.H, c.W), np.float32)
            ctx.call("r3d_wls_filter_dev", ctypes.byref(p), _vp(ptrs[0]), _vp(ptrs[1]), _vp(ptrs[2]), 1, c.W, c.W, c.H, _vp(ptrs[3]),
                     _vp(ptrs[4]))
            ctx.d2h(out, ptrs[3])
            ctx.d2h(conf, ptrs[4])
            np.testing.assert_array_equal(out, want)
            np.testing.assert_array_equal(conf, wconf)
            ctx.call("r3d_wls_filter_dev", ctypes.byref(p), _vp(ptrs[0]), _vp(ptrs[1]), _vp(ptrs[2]), 1, c.W, c.W, c.H, _vp(ptrs[3]), None)
            ctx.d2h(out, ptrs[3])
            np.testing.assert_array_equal(out, want)              # without a confidence output
    finally:
        for q in ptrs:
            ctx.free(q)


# ------------------------------------------------------------------------------------------------------ normalize

SWEEP = 1024 * 256 * 8       # elements one pass of k_minmax_s16's capped grid covers


def _norm_array(n, seed):
    a = np.random.default_rng(seed).integers(-1000, 1001, n).astype(np.int16)
    if n > 1:
        a[-1] = -5000                                             # the only minimum
        a[SWEEP + 5 if n > SWEEP + 5 else n - 2] = 6000           # the only maximum (second sweep where the array has one)
    return a


@pytest.mark.parametrize("n", [1, 2, 7, 8, 9, 2047, 2048, 2049, 2097151, 2099201, 3000001])
def test_normalize_sizes_and_grid_stride(r3d, n):
    """Above SWEEP elements the extremes sit where only the grid-stride iterations of the min/max kernel read."""
    a = _norm_array(n, n)
    got = r3d.normalize(a, None, 0, 255)
    want = _po().normalize_minmax(a)
    np.testing.assert_array_equal(got, want)
    if n > 1:
        assert want.min() == 0 and want.max() == 255 and (want == 255).sum() == 1 and (want == 0).sum() == 1


@pytest.mark.parametrize("alpha,beta", [(0, 255), (255, 0), (10, 10), (-300, 300), (0, 40000)])
def test_normalize_ranges_extremes_and_constant(r3d, alpha, beta):
    po = _po()
    rng = np.random.default_rng(7)
    full = rng.integers(-32768, 32768, 2049).astype(np.int16)
    full[3], full[2040] = -32768, 32767
    mid = _norm_array(2049, 8)
    const = np.full(300, -3, np.int16)
    for a in (full, mid, const):
        np.testing.assert_array_equal(r3d.normalize(a, None, alpha, beta), po.normalize_minmax(a, alpha, beta))
    if (alpha, beta) == (0, 40000):
        assert r3d.normalize(full, None, alpha, beta).max() == 32767 and (po.normalize_minmax(full, alpha, beta) == 32767).sum() > 100
    assert (r3d.normalize(const, None, alpha, beta) == min(alpha, beta)).all()


@pytest.mark.parametrize("off", [1, 3, 7])
def test_normalize_dev_unaligned_head(r3d, off):
    """Pointers offset by off int16 into an allocation: (8 - off) elements precede the first 16-byte boundary and only the
    scalar head loop of the min/max kernel reads them; both extremes are put there (or, with a head of one, one of them)."""
    po = _po()
    ctx = r3d.default_context()
    n, head = 5000, 8 - off
    d_src, d_dst = ctx.alloc((n + 16) * 2), ctx.alloc((n + 16) * 2)
    try:
        assert d_src % 16 == 0 and d_dst % 16 == 0
        for lo_at, hi_at in ((0, head - 1 if head > 1 else n - 1), (head - 1 if head > 1 else n - 1, 0)):
            a = np.random.default_rng(off).integers(-1000, 1001, n).astype(np.int16)
            a[lo_at], a[hi_at] = -5000, 6000
            guard = np.full(n + 16, 777, np.int16)
            ctx.h2d(d_dst, guard)
            ctx.h2d(d_src, guard)
            ctx.h2d(d_src + 2 * off, a)
            ctx.call("r3d_normalize_minmax_s16_dev", _vp(d_src + 2 * off), ctypes.c_int64(n), 0.0, 255.0, _vp(d_dst + 2 * off))
            back = np.empty(n + 16, np.int16)
            ctx.d2h(back, d_dst)
            np.testing.assert_array_equal(back[off:off + n], po.normalize_minmax(a))
            assert (back[:off] == 777).all() and (back[off + n:] == 777).all()      # nothing written outside [off, off + n)
    finally:
        ctx.free(d_src)
        ctx.free(d_dst)


# ---------------------------------------------------------------------------------------------------------- remap

def _remap_padded(r3d, img, pad, m1, m2, border=0, with_gray=False):
    """img uint8 [sh, sw] or [sh, sw, cn] -> r3d_remap_u8 with a row stride of sw * cn + pad bytes, padding filled with 255."""
    sh, sw = img.shape[:2]
    cn = 1 if img.ndim == 2 else img.shape[2]
    buf = np.full((sh, sw * cn + pad), 255, np.uint8)
    buf[:, :sw * cn] = img.reshape(sh, sw * cn)
    dh, dw = m2.shape
    m1, m2 = np.ascontiguousarray(m1), np.ascontiguousarray(m2)
    dst = np.full((dh, dw) if img.ndim == 2 else (dh, dw, cn), 99, np.uint8)
    gray = np.full((dh, dw), 99, np.uint8) if with_gray else None
    r3d.default_context().call("r3d_remap_u8", _p(buf), sw, sh, sw * cn + pad, cn, _p(m1), _p(m2), dw, dh, int(border), _p(dst),
                               _p(gray) if with_gray else None)
    return (dst, gray) if with_gray else dst


def _maps(rng, sw, sh, dw, dh, reach=3):
    m1 = np.stack([rng.integers(-reach, sw + reach, (dh, dw)), rng.integers(-reach, sh + reach, (dh, dw))], -1).astype(np.int16)
    m2 = rng.integers(0, 1024, (dh, dw)).astype(np.uint16)
    m2[::2, ::3] = 0
    return m1, m2


@pytest.mark.parametrize("cn", [1, 3, 4])
def test_remap_padded_source_stride(r3d, cn):
    """sstride > sw * cn: a kernel that steps rows by sw * cn, or reads one tap past a row's end, picks up the 255 padding."""
    rng = np.random.default_rng(20 + cn)
    sh, sw = 23, 37
    img = rng.integers(0, 200, (sh, sw) if cn == 1 else (sh, sw, cn), dtype=np.uint8)
    m1, m2 = _maps(rng, sw, sh, 61, 19)
    m1[0, :sw, 0], m1[0, :sw, 1] = np.arange(sw), 5                  # includes sx = sw - 1: the right tap is the border
    np.testing.assert_array_equal(_remap_padded(r3d, img, 7, m1, m2, border=3), _po().remap_fixed(img, m1, m2, border_value=3))
    np.testing.assert_array_equal(_remap_padded(r3d, img, 0, m1, m2, border=3), _po().remap_fixed(img, m1, m2, border_value=3))


@pytest.mark.parametrize("dw", [255, 256, 257])
def test_remap_destination_width_around_the_block(r3d, dw):
    rng = np.random.default_rng(dw)
    img = rng.integers(0, 256, (11, 13, 3), dtype=np.uint8)
    m1, m2 = _maps(rng, 13, 11, dw, 3)
    np.testing.assert_array_equal(r3d.remap(img, m1, m2), _po().remap_fixed(img, m1, m2))


@pytest.mark.parametrize("sw,sh", [(1, 1), (1, 40), (40, 1)])
@pytest.mark.parametrize("cn", [1, 3])
def test_remap_one_pixel_wide_sources(r3d, sw, sh, cn):
    rng = np.random.default_rng(sw * 100 + sh + cn)
    img = rng.integers(1, 256, (sh, sw) if cn == 1 else (sh, sw, cn), dtype=np.uint8)
    m1, m2 = _maps(rng, sw, sh, 70, 9, reach=2)
    want = _po().remap_fixed(img, m1, m2, border_value=9)
    np.testing.assert_array_equal(r3d.remap(img, m1, m2, borderValue=9), want)
    np.testing.assert_array_equal(_remap_padded(r3d, img, 7, m1, m2, border=9), want)
    assert (want != 9).mean() > 0.05


def test_remap_map_entries_at_the_int16_limits(r3d):
    rng = np.random.default_rng(31)
    img = rng.integers(0, 256, (9, 14), dtype=np.uint8)
    m1, m2 = _maps(rng, 14, 9, 40, 6)
    for k, (vx, vy) in enumerate([(-32768, 2), (32767, 2), (3, -32768), (3, 32767), (-32768, -32768), (32767, 32767), (-32768, 32767)]):
        m1[k % 6, 5 * (k // 6) + k] = (vx, vy)
    got = r3d.remap(img, m1, m2, borderValue=200)
    np.testing.assert_array_equal(got, _po().remap_fixed(img, m1, m2, border_value=200))
    assert got[0, 0] == 200 and got[1, 1] == 200


def test_remap_fused_gray_from_four_channels(r3d):
    rng = np.random.default_rng(32)
    po = _po()
    img = rng.integers(0, 256, (17, 29, 4), dtype=np.uint8)
    m1, m2 = _maps(rng, 29, 17, 257, 5)
    for pad in (0, 7):
        dst, gray = _remap_padded(r3d, img, pad, m1, m2, border=77, with_gray=True)
        want = po.remap_fixed(img, m1, m2, border_value=77)
        np.testing.assert_array_equal(dst, want)
        np.testing.assert_array_equal(gray, po.bgr2gray(want))
    assert (gray == 77).any() and (gray != 77).any()


# --------------------------------------------------------------------------------------------------- rectify maps

_K = np.array([[62.0, 0, 20.25], [0, 60.0, 31.5], [0, 0, 1]])       # short focal length: r2 reaches 0.5, every term counts
_PN = np.array([[58.0, 0, 21.0], [0, 58.0, 30.0], [0, 0, 1]])
_DIST = np.array([0.12, -0.2, 1e-3, -2e-3, 0.04, 0.01, -0.02, 0.003, 1e-3, -1e-3, 2e-3, 5e-4, 0.0, 0.0])


def _rot():
    a, b = 0.02, -0.015
    Rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    Ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    return Rx @ Ry


@pytest.mark.parametrize("size", [(7, 1), (1, 63), (40, 64), (40, 65)])
@pytest.mark.parametrize("n_dist", [0, 4, 8, 14])
def test_rectify_maps_distortion_lengths_and_row_counts(r3d, n_dist, size):
    dist = None if n_dist == 0 else _DIST[:n_dist]
    R = _rot()
    a1, a2 = r3d.initUndistortRectifyMap(_K, dist, R, _PN, size)
    b1, b2 = _po().init_undistort_rectify_map(_K, dist, R, _PN, size)
    assert a1.shape == (size[1], size[0], 2) and a2.shape == (size[1], size[0])
    np.testing.assert_array_equal(a1, b1)
    np.testing.assert_array_equal(a2, b2)


def test_rectify_maps_distortion_terms_matter_and_p_3x4_equals_3x3(r3d):
    size = (40, 65)
    R = _rot()
    P4 = np.hstack([_PN, [[-58.0 * 0.12], [1.5], [0.25]]])          # the fourth column is not part of the map
    maps = {}
    for n_dist in (0, 4, 8, 14):
        dist = None if n_dist == 0 else _DIST[:n_dist]
        a1, a2 = r3d.initUndistortRectifyMap(_K, dist, R, _PN, size)
        c1, c2 = r3d.initUndistortRectifyMap(_K, dist, R, P4, size)
        np.testing.assert_array_equal(a1, c1)
        np.testing.assert_array_equal(a2, c2)
        maps[n_dist] = a2
    assert (maps[0] != maps[4]).any() and (maps[4] != maps[8]).any() and (maps[8] != maps[14]).any()
