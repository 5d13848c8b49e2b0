"""GPU tests of resource ownership (csrc/r3d_resources.h) through the live counts of r3d_debug_resources: whatever a context, a
resident model or a TSDF volume allocates is gone once it is destroyed, and a buffer that grows frees what it replaces.  Every
test uses contexts of its own (the default context lives on with whatever the other modules made it allocate) and compares
differences of the process-wide counts, never their values.

Not tested here: the failure paths (tools/cpu_sanitize_resources.sh walks them on a machine without a GPU; exhausting a shared
card's memory is not an option), and the poisoned-context refusal of the pre/post stages (the suite has no way to poison a
context that does not leave work hanging on the card; the same program checks the arena's refusal for both buffer lists)."""
import ctypes

import numpy as np
import pytest

from tests import rgbd_scene as sc

pytestmark = pytest.mark.gpu
FIELDS = ("device_allocs", "device_bytes", "pinned_allocs", "events", "streams")
VL, TRUNC = 0.01, 0.04
POSES = (np.eye(4), sc.TRUTH, sc.pose(-2, 3, 1, (0.05, 0.03, -0.04)))     # test_tsdf_gpu's case A: a pool of 8 units grows to 240


def _diff(a, b):
    return {k: a[k] - b[k] for k in FIELDS}


def _sgbm(r3d, ctx, mode, **kw):
    m = r3d.StereoSGBM(minDisparity=0, numDisparities=16, blockSize=5, P1=8 * 25, P2=32 * 25, disp12MaxDiff=1, uniquenessRatio=10,
                       mode=mode, **kw)
    m._ctx = ctx
    return m


def _grown_volume(r3d, ctx, initial_units=8):
    """a colour volume fed case A's three frames"""
    vol = r3d.ScalableTSDFVolume(VL, TRUNC, r3d.TSDFVolumeColorType.RGB8, depth_sampling_stride=4, initial_units=initial_units, ctx=ctx)
    cam = sc.camera(64, 48)
    for pose in POSES:
        inten, depth = sc.render(64, 48, pose, sc.HOLES)
        color = np.ascontiguousarray(np.repeat((inten * 255).astype(np.uint8)[..., None], 3, axis=2))
        vol.integrate_f32(depth, color, cam, np.linalg.inv(pose))
    return vol


def _held_by(r3d, thing):
    """what closing `thing` gives back"""
    before = r3d._lib.live_resources()
    thing.close()
    return _diff(before, r3d._lib.live_resources())


def test_lifecycle_balance(r3d, synth):
    live = r3d._lib.live_resources
    co = r3d.cloud_ops
    snap = live()
    ctx = r3d.Context(0)
    # stereo: both modes through the host entry point, once with profiling on (the lazily created event ring)
    L, R, _ = synth.stereo_pair(64, 48, 16, seed=3)
    m = _sgbm(r3d, ctx, r3d.stereo_sgbm.STEREO_SGBM_MODE_SGBM_3WAY)
    ctx.set_profiling(True)
    dl = m.compute(L, R)
    assert ctx.sgbm_profile()
    ctx.set_profiling(False)
    _sgbm(r3d, ctx, r3d.stereo_sgbm.STEREO_SGBM_MODE_HH).compute(L, R)
    # four maps over three lanes: lane streams, their `done` events and the fork event; lane 0 is used twice
    batch = m.compute_batch([L] * 4, [R] * 4)
    assert all(np.array_equal(b, dl) for b in batch)
    # speckle filter and the pre/post stages (pp_bufs, pp_lut, pp_minmax)
    spk = np.ascontiguousarray(dl.copy())
    ctx.call("r3d_filter_speckles", spk.ctypes.data_as(ctypes.c_void_p), 64, 48, 0, 50, 32)
    rm = r3d.stereo_sgbm.createRightMatcher(m)
    rm._ctx = ctx
    wls = r3d.stereo_prepost.DisparityWLSFilter(0, 16, 5)
    wls._ctx = ctx
    filtered = wls.filter(dl, L, disparity_map_right=rm.compute(R, L))
    r3d.stereo_prepost.normalize(filtered, ctx=ctx)
    # clouds: the arena, the pinned read-back block and the registration's pinned state
    rng = np.random.default_rng(5)
    pts = rng.random((400, 3)) * 0.2
    T = sc.pose(1.0, -1.0, 0.5, (0.004, -0.003, 0.002))
    moved = pts @ T[:3, :3].T + T[:3, 3]
    co.voxel_down_sample(pts, 0.02, ctx=ctx)
    nrm = co.estimate_normals(pts, 0.05, 30, ctx=ctx)
    co.registration(pts, moved, 0.05, mode=co.P2P, max_iteration=5, ctx=ctx)
    # resident model: rows, both voxel tables (the second frame merges into the first frame's table) and the pending box
    model = co.ResidentModel(ctx)
    model.append(pts)
    model.align_append(moved, threshold=0.05, voxel_size=0.01, max_iteration=5)
    model.align_append(moved + 0.001, threshold=0.05, voxel_size=0.01, max_iteration=5)
    # the three entry points with events of their own
    d_p, d_n, d_f = ctx.to_device(pts), ctx.to_device(nrm), ctx.alloc(400 * 33 * 8)
    co.debug_fpfh_stages(d_p, d_n, 400, 0.05, d_f, max_nn=30, ctx=ctx)
    for d in (d_p, d_n, d_f):
        ctx.free(d)
    ms = ctypes.c_float()
    ctx.call("r3d_debug_streambench", 0, 4, ctypes.c_uint64(4096), 1, 0, 1, ctypes.byref(ms))
    src, tgt, cam, _ = sc.pair(67, 45)
    co.rgbd_odometry(src, tgt, cam, ctx=ctx)
    # a volume that grows, and an extraction
    vol = _grown_volume(r3d, ctx)
    assert vol.stats()["growths"] >= 3
    assert vol.point_count() > 0

    alive = _diff(live(), snap)
    print("alive:", alive)
    assert all(alive[k] > 0 for k in FIELDS), alive          # the counters are wired
    assert alive["streams"] == 4 and alive["pinned_allocs"] == 3
    model.close()
    vol.close()
    ctx.close()
    assert live() == snap


def test_growth_frees_what_it_replaces(r3d, synth):
    ctx = r3d.Context(0)
    grown = _grown_volume(r3d, ctx)
    st = grown.stats()
    assert st["growths"] >= 3
    fresh = _grown_volume(r3d, ctx, initial_units=st["capacity"])
    assert fresh.stats()["growths"] == 0 and fresh.stats()["capacity"] == st["capacity"]
    a, b = _held_by(r3d, grown), _held_by(r3d, fresh)
    print("volume grown to", st["capacity"], "units holds", a, "- created at that size", b)
    assert a["device_allocs"] > 0 and a["device_bytes"] > st["capacity"] * 4096 * 8
    assert (a["device_bytes"], a["device_allocs"]) == (b["device_bytes"], b["device_allocs"])
    assert _held_by(r3d, ctx)["streams"] == 1

    held = []
    for sizes in (((64, 48), (128, 96)), ((128, 96),)):
        ctx = r3d.Context(0)
        m = _sgbm(r3d, ctx, r3d.stereo_sgbm.STEREO_SGBM_MODE_SGBM_3WAY)
        for w, h in sizes:
            L, R, _ = synth.stereo_pair(w, h, 16, seed=3)
            m.compute(L, R)
        held.append(_held_by(r3d, ctx))
    print("context after 64x48 then 128x96:", held[0], "- after 128x96 alone:", held[1])
    assert held[0]["device_bytes"] > 0 and held[0]["device_bytes"] == held[1]["device_bytes"]
