"""Coloured clouds from stereo views: r3d_disparity_to_cloud_color_dev / _resident and the pipeline functions on top of them.
The colour image is random uint8 (a wrong pixel or channel cannot pass by accident) and is not the matched image.  Colours are
compared exactly: (double)byte / 255.0 of the source pixel, voxel means summed in member order as the oracle sums them."""
import os

import numpy as np
import pytest

from oracle import cloud_oracle as co
from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu

W, H, D = 200, 120, 32
MAX_DEPTH = 0.4                     # drops the far ~10 % of this pair's points
VOXEL_SMALL, VOXEL_BIG = 0.004, 0.03     # ~2 members per voxel / ~40 with some twenty voxels above VM_BIG (oracle counts, seed 5)
VM_BIG = 192                        # csrc/cloud.hip: voxels with more members are summed by a wave each


def _Q(r3d, width):
    return r3d.pipeline.scaled_Q(np.load(os.path.join(GOLDEN, "jetson_stereo_8MP_stereo.npz"))["Q"], width / 960.0, unit=1e-3)


@pytest.fixture(scope="module")
def view(r3d, synth):
    """One matched 200 x 120 pair: the disparity map left on the device and read back, with the pixels of its valid points."""
    m = r3d.reference_matcher(numDisparities=D, blockSize=5)
    ctx = m.context
    L, R, _ = synth.stereo_pair(W, H, D, seed=5)
    d_l, d_r, d_d = ctx.to_device(L), ctx.to_device(R), ctx.alloc(W * H * 2)
    m.compute_device(d_l, d_r, W, H, W, d_d)
    disp = np.empty((H, W), np.int16)
    ctx.d2h(disp, d_d)
    Q = _Q(r3d, W)
    pts, pix = r3d.cloud_ops.reproject_disparity(disp, Q, 0, want_pixels=True)
    yield dict(m=m, ctx=ctx, L=L, R=R, Q=Q, d_d=d_d, disp=disp, pts=pts, pix=pix)
    for p in (d_l, d_r, d_d):
        ctx.free(p)


def _image(cn, seed=0):
    img = np.random.default_rng(100 + seed).integers(0, 256, (H, W, cn) if cn == 3 else (H, W), dtype=np.uint8)
    return img


def _expected(img, pix, order):
    """colours of the pixels `pix` of a host image, r, g, b"""
    c = img.reshape(H * W, -1)[pix] / 255.0
    if c.shape[1] == 1:
        return np.repeat(c, 3, 1)
    return c[:, ::-1] if order == "bgr" else c


def _lex(p):
    return np.lexsort(p.T[::-1])


@pytest.mark.parametrize("cn,order,pad", [(1, "bgr", 0), (3, "bgr", 0), (3, "rgb", 0), (3, "bgr", 7), (1, "rgb", 5)])
def test_raw_gather_equals_the_pixels_of_the_image(r3d, view, cn, order, pad):
    """voxel grid and normals off: one colour per valid pixel; pad > 0: a device image whose rows are further apart than W * cn"""
    ctx, img = view["ctx"], _image(cn)
    up = img.reshape(H, W * cn)
    if pad:
        up = np.concatenate([up, np.full((H, pad), 255 if cn == 1 else 0, np.uint8)], 1)     # padding that is no valid colour source
    d_c = ctx.to_device(up)
    try:
        pts, nrm, col = r3d.cloud_ops.disparity_to_cloud_device(view["d_d"], W, H, view["Q"], 0, None, None, 0, None, 0, ctx=ctx, d_color=d_c,
                                                                color_stride=W * cn + pad, color_channels=cn, color_order=order)
        plain, _ = r3d.cloud_ops.disparity_to_cloud_device(view["d_d"], W, H, view["Q"], 0, None, None, 0, None, 0, ctx=ctx)
    finally:
        ctx.free(d_c)
    keep = np.isfinite(view["pts"]).all(1)                     # the chain drops points at infinity (W = 0)
    assert nrm is None and len(pts) == keep.sum() > 10000
    np.testing.assert_array_equal(pts, plain)
    np.testing.assert_array_equal(pts, view["pts"][keep])
    np.testing.assert_array_equal(col, _expected(img, view["pix"][keep], order))
    if cn == 3:
        assert not np.array_equal(col, col[:, ::-1])


@pytest.mark.parametrize("voxel", [VOXEL_SMALL, VOXEL_BIG])
@pytest.mark.parametrize("cn", [1, 3])
def test_voxel_mean_colours_equal_the_oracle_bit_for_bit(r3d, view, voxel, cn):
    """The voxel-mean kernels read the bytes through pix and idx and sum in member order: the oracle's voxel_down_sample on the
    library's own pre-voxel points and gathered colours must give the same bits.  VOXEL_BIG has voxels above VM_BIG members (the
    wave-per-voxel kernel) with counts that are no multiple of 64; both sizes have counts that are no multiple of 8."""
    ctx, img = view["ctx"], _image(cn, seed=1)
    d_c = ctx.to_device(img)
    kw = dict(ctx=ctx, d_color=d_c, color_channels=cn, color_order="bgr")
    try:
        raw_p, _, raw_c = r3d.cloud_ops.disparity_to_cloud_device(view["d_d"], W, H, view["Q"], 0, MAX_DEPTH, None, 0, None, 0, **kw)
        got_p, _, got_c = r3d.cloud_ops.disparity_to_cloud_device(view["d_d"], W, H, view["Q"], 0, MAX_DEPTH, None, voxel, None, 0, **kw)
        plain_p, _ = r3d.cloud_ops.disparity_to_cloud_device(view["d_d"], W, H, view["Q"], 0, MAX_DEPTH, None, voxel, None, 0, ctx=ctx)
    finally:
        ctx.free(d_c)
    assert 10000 < len(raw_p) < np.isfinite(view["pts"]).all(1).sum()          # the depth filter is on and drops some
    _, cnt = np.unique(co.voxel_keys(raw_p, voxel), axis=0, return_counts=True)
    small, big = cnt[cnt <= VM_BIG], cnt[cnt > VM_BIG]
    assert (small % 8 != 0).any()                                  # the remainder path of the thread-per-voxel kernel
    if voxel == VOXEL_SMALL:
        assert len(big) == 0 and 1.5 < cnt.mean() < 8
    else:
        assert len(big) >= 2 and (big % 64 != 0).any()             # the wave-per-voxel kernel and its remainder path
    want_p, want_c = co.voxel_down_sample(raw_p, voxel, raw_c)
    assert len(got_p) == len(want_p) == len(cnt)
    np.testing.assert_array_equal(got_p, plain_p)
    ia, ib = _lex(got_p), _lex(want_p)
    np.testing.assert_array_equal(got_p[ia], want_p[ib])
    np.testing.assert_array_equal(got_c[ia], want_c[ib])
    assert got_c.min() >= 0.0 and got_c.max() <= 1.0 and len(np.unique(got_c)) > 100


def test_view_to_cloud_chains_agree_with_and_without_colour(r3d, synth, view):
    m, L, R, Q = view["m"], view["L"], view["R"], view["Q"]
    pose = synth.rigid((0.2, 1, 0.1), 3.0, (0.01, -0.02, 0.005))
    kw = dict(voxel=VOXEL_SMALL, pose=pose, max_depth=MAX_DEPTH, max_nn=20)
    img = _image(3, seed=2)
    a = r3d.pipeline.view_to_cloud(L, R, Q, m, device_resident=True, color=img, **kw)
    b = r3d.pipeline.view_to_cloud(L, R, Q, m, device_resident=False, color=img, **kw)
    c = r3d.pipeline.view_to_cloud(L, R, Q, m, device_resident=True, color=None, **kw)
    assert len(a) > 1000 and a.has_colors() and a.has_normals() and not c.has_colors()
    for x in (b, c):
        np.testing.assert_array_equal(a.points, x.points)
        np.testing.assert_array_equal(a.normals, x.normals)
    np.testing.assert_array_equal(a.colors, b.colors)
    # color=True: the left image itself, grey -> r = g = b
    for resident in (True, False):
        g = r3d.pipeline.view_to_cloud(L, R, Q, m, device_resident=resident, color=True, **kw)
        np.testing.assert_array_equal(g.points, a.points)
        assert g.has_colors() and np.array_equal(g.colors[:, 0], g.colors[:, 1]) and np.array_equal(g.colors[:, 0], g.colors[:, 2])
    # an [H,W,3] BGR pair with color=True: colours come back as r, g, b
    L3 = np.ascontiguousarray(np.stack([L, L // 2, 255 - L], -1))
    R3 = np.ascontiguousarray(np.stack([R, R // 2, 255 - R], -1))
    p3 = r3d.pipeline.view_to_cloud(L3, R3, Q, m, device_resident=True, color=True, voxel=0, max_depth=MAX_DEPTH, max_nn=0)
    disp3 = m.compute(L3, R3)
    pts3, pix3 = r3d.cloud_ops.reproject_disparity(disp3, Q, 0, want_pixels=True)
    keep = np.abs(pts3[:, 2]) <= MAX_DEPTH
    assert len(p3) == keep.sum() > 1000 and not p3.has_normals()
    np.testing.assert_array_equal(p3.points, pts3[keep])
    np.testing.assert_array_equal(p3.colors, L3.reshape(-1, 3)[pix3[keep]][:, ::-1] / 255.0)
    a3 = r3d.pipeline.view_to_cloud(L3, R3, Q, m, device_resident=True, color=True, **kw)
    b3 = r3d.pipeline.view_to_cloud(L3, R3, Q, m, device_resident=False, color=True, **kw)
    assert len(a3) > 1000
    for f in ("points", "normals", "colors"):
        np.testing.assert_array_equal(getattr(a3, f), getattr(b3, f))


TW, TH, TD = 320, 200, 32


def test_tensor_chains_and_fusion_carry_the_colour_plane(r3d, synth):
    import torch
    Q = _Q(r3d, TW)
    m = r3d.reference_matcher(numDisparities=TD, blockSize=5)
    ctx = m.context
    kw = dict(voxel=0.004, max_nn=20, max_depth=0.5)
    cap = TW * TH
    views = []
    for v in (0, 1):
        L, R, _ = synth.stereo_pair(TW, TH, TD, seed=40 + v)
        img = np.random.default_rng(7 + v).integers(0, 256, (TH, TW, 3), dtype=np.uint8)
        views.append((torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda(), torch.from_numpy(img).cuda()))
    poses = [np.eye(4), np.linalg.inv(synth.rigid((0.2, 1.0, 0.1), 0.3, (0.0025, -0.0015, 0.001)))]
    d_disp = torch.empty(TW * TH, dtype=torch.int16, device="cuda")
    single = []
    for v, (tl, tr, tc) in enumerate(views):
        out = torch.empty((3, cap, 3), dtype=torch.float64, device="cuda")
        got = r3d.pipeline.view_to_cloud_tensors(tl.data_ptr(), tr.data_ptr(), d_disp.data_ptr(), TW, TH, Q, m, out, pose=poses[v],
                                                 d_color=tc.data_ptr(), **kw)
        torch.cuda.synchronize()
        # d_disp holds this view's map: the host-output call on it
        p, n, c = r3d.cloud_ops.disparity_to_cloud_device(d_disp.data_ptr(), TW, TH, Q, 0, kw["max_depth"], poses[v], kw["voxel"],
                                                          2 * kw["voxel"], kw["max_nn"], ctx=ctx, d_color=tc.data_ptr())
        assert got.shape == (3, len(p), 3) and len(p) > 1000
        np.testing.assert_array_equal(got.cpu().numpy(), np.stack([p, n, c]))
        single.append(got.clone())
        with pytest.raises(ValueError):
            r3d.pipeline.view_to_cloud_tensors(tl.data_ptr(), tr.data_ptr(), d_disp.data_ptr(), TW, TH, Q, m, out[:2], pose=poses[v],
                                               d_color=tc.data_ptr(), **kw)
    cctx = r3d.Context(ctx.device)
    try:
        disps = [torch.empty(TW * TH, dtype=torch.int16, device="cuda") for _ in views]
        outs = [torch.empty((3, cap, 3), dtype=torch.float64, device="cuda") for _ in views]
        piped = r3d.pipeline.views_to_cloud_tensors([(a.data_ptr(), b.data_ptr()) for a, b, _ in views], [d.data_ptr() for d in disps], TW, TH, Q,
                                                    m, outs, cctx, poses=poses, d_colors=[c.data_ptr() for _, _, c in views], **kw)
        torch.cuda.synchronize()
        for v in (0, 1):
            assert torch.equal(piped[v], single[v])
        with pytest.raises(ValueError):
            r3d.pipeline.views_to_cloud_tensors([(a.data_ptr(), b.data_ptr()) for a, b, _ in views], [d.data_ptr() for d in disps], TW, TH, Q,
                                                m, [o[:2] for o in outs], cctx, poses=poses, d_colors=[c.data_ptr() for _, _, c in views], **kw)
    finally:
        cctx.close()
    local3 = {v: single[v] for v in (0, 1)}
    local2 = {v: single[v][:2].contiguous() for v in (0, 1)}
    fused3, T3 = r3d.pipeline.multi_view_fuse_tensors(local3, 2, threshold=0.02, max_iteration=10)
    fused2, T2 = r3d.pipeline.multi_view_fuse_tensors(local2, 2, threshold=0.02, max_iteration=10)
    assert fused3.shape == (3, single[0].shape[1] + single[1].shape[1], 3) and fused2.shape[0] == 2
    assert torch.equal(fused3[2], torch.cat([single[0][2], single[1][2]]))
    assert torch.equal(fused3[:2], fused2) and np.array_equal(T3[1], T2[1])
    with pytest.raises(ValueError):
        r3d.pipeline.multi_view_fuse_tensors({0: local3[0], 1: local2[1]}, 2, threshold=0.02, max_iteration=10)


def test_edges_and_refusals(r3d, view):
    ctx, Q = view["ctx"], view["Q"]
    img = _image(3, seed=3)
    d_c = ctx.to_device(img)
    d_bad = ctx.to_device(np.full((H, W), -16, np.int16))             # the matcher's invalid marker everywhere
    d_out = ctx.alloc(24)
    call = r3d.cloud_ops.disparity_to_cloud_device
    try:
        p, n, c = call(d_bad, W, H, Q, 0, None, None, 0.01, None, 10, ctx=ctx, d_color=d_c)
        assert p.shape == (0, 3) and c.shape == (0, 3)
        with pytest.raises(r3d.R3DError, match="output arrays hold"):
            call(view["d_d"], W, H, Q, 0, None, None, 0, None, 0, capacity=10, ctx=ctx, d_color=d_c)
        with pytest.raises(r3d.R3DError, match="channels"):
            call(view["d_d"], W, H, Q, 0, None, None, 0, None, 0, ctx=ctx, d_color=d_c, color_channels=2, color_stride=3 * W)
        with pytest.raises(r3d.R3DError, match="stride"):
            call(view["d_d"], W, H, Q, 0, None, None, 0, None, 0, ctx=ctx, d_color=d_c, color_stride=3 * W - 1)
        with pytest.raises(r3d.R3DError, match="output array for the colours"):
            r3d.cloud_ops.disparity_to_cloud_resident(view["d_d"], W, H, Q, d_out, None, 1, max_nn=0, ctx=ctx, d_color=d_c, d_out_colors=None)
        with pytest.raises(ValueError):
            call(view["d_d"], W, H, Q, 0, None, None, 0, None, 0, ctx=ctx, d_color=d_c, color_order="gbr")
    finally:
        for p in (d_c, d_bad, d_out):
            ctx.free(p)
    m, L, R = view["m"], view["L"], view["R"]
    for bad in (img[:-1], img[:, :, :2], img.astype(np.float32), img.astype(np.int16), np.zeros((H, W, 3, 1), np.uint8)):
        for resident in (True, False):
            with pytest.raises(ValueError):
                r3d.pipeline.view_to_cloud(L, R, Q, m, device_resident=resident, color=bad)
    with pytest.raises(ValueError):
        r3d.pipeline.view_to_cloud(L, R, Q, m, color=True, color_order="gbr")
