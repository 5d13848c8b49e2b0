"""Orchestration counterparts of the reference's per-frame loops, on top of the HIP-backed stage classes.

fuse()             main.py:34-54 simple_scanning_loop (and test/GICP1.py:134-155): skip empty frames, first valid frame
                   initialises the model, every later frame is aligned to the model and appended.
view_to_cloud()    the join the reference never wrote (Q is loaded at Calib_depth/depth2.py:66 and then unused):
                   StereoSGBM disparity -> reprojectImageTo3D -> voxel_down_sample -> normals.
multi_view_fuse_tensors()  BASELINE config C5: one view per rank, ONE all-gather-v of the per-view clouds (RCCL, clouds stay in
                   HBM), every view registered to view 0, fused cloud on every rank (rank 0 hands it to the mesher,
                   mesh_reconstruction.py:22-37); multi_view_fuse() is its host-cloud front end.
"""
import ctypes

import numpy as np

from . import cloud_ops, distributed, tsdf
from .pointcloud import PointCloud, as_arrays
from .pointcloud_alignment import GeneralizedICPAlignment, PointCloudAlignment


def fuse(frames, flavour="icp", verbose=False, resident=True, ctx=None, log=None, **align_kw):
    """frames: iterable of PointCloud-likes (or None / empty for a failed capture).  Returns the accumulated model.
    flavour "icp": main.py:34-54 (align_point_clouds(frame, model, threshold=0.02, voxel_size=0.01, max_iter=100), model += aligned);
    flavour "gicp": test/GICP1.py:134-155 (registration_generalized_icp of the frame against the whole model, model += aligned,
    model.estimate_normals(Hybrid(0.05, 30))).  align_kw: threshold / voxel_size / max_iter (icp), threshold (gicp).
    resident (default): the model stays in HBM across frames (cloud_ops.ResidentModel): per frame only the frame goes up and the
    4x4 comes back, the model is downloaded once at the end.  resident=False drives the drop-in classes with a host-side model
    exactly as the reference's loop does (identical results; every frame then re-uploads the whole model).
    `log` (list) receives the registration result of every aligned frame."""
    if not resident:
        return _fuse_host(frames, flavour, verbose, log, **align_kw)
    model = first = None
    for frame in frames:
        if frame is None or len(as_arrays(frame)[0]) == 0:
            if verbose:
                print("No valid point cloud captured, skipping frame.")      # main.py:53-54
            continue
        p, c, n = as_arrays(frame)
        if first is None:
            # main.py:42-45: points + colors only; GICP1.py:139-141: normals as well.  Stays on the host until a second
            # frame needs a model to register against (a one-frame scan never touches the GPU)
            first = (p.copy(), None if c is None else c.copy(), n.copy() if (flavour == "gicp" and n is not None) else None)
            continue
        if model is None:
            model = cloud_ops.ResidentModel(ctx)
            model.append(*first)
        if flavour == "icp":
            if verbose:                                                      # the three progress lines of align_point_clouds
                print("Downsampling point clouds using voxel size:", align_kw.get("voxel_size", 0.01))
                print("Estimating normals on CPU...")
                print("Performing ICP alignment using CUDA...")
            vs = align_kw.get("voxel_size", 0.01)
            res = model.align_append(p, align_kw.get("threshold", 0.02), vs, align_kw.get("max_iter", 100), cloud_ops.P2P, 2 * vs, 30,
                                     source_colors=c)
        else:
            if n is None:                                                    # GICP1.py:94-95
                n = cloud_ops.estimate_normals(p, 0.05, 30, ctx=ctx)
            if not model.size()[2]:                                          # GICP1.py:96-97
                model.estimate_normals(0.05, 30)
            res = model.register_append(p, align_kw.get("threshold", 0.02), cloud_ops.GICP, 30, source_colors=c, source_normals=n)
            model.estimate_normals(0.05, 30)                                 # GICP1.py:148
        if log is not None:
            log.append(res)
    if model is None:
        return PointCloud(*((first[0], first[1], first[2]) if first is not None else ()))
    pts, cols, nrm = model.download()
    model.close()
    return PointCloud(pts, cols, nrm)


def fuse_depth_frames(depth_images, camera, colors=None, verbose=False, ctx=None, log=None, threshold=0.02, voxel_size=0.01, max_iter=100):
    """main.py:34-54 for frames that arrive as depth images (the recorded test/output84 frames; a RealSense z16 frame):
    create_from_rgbd_image + flip (test/check84.py:155-159,172-178) runs on the device, the model stays in HBM, the frame that
    crosses PCIe is the 0.6 MB image.  depth_images: iterable of uint16 [H,W] arrays (None / all-invalid = failed capture,
    skipped); camera: cloud_ops.depth_camera(intrinsics); colors: optional iterable of uint8 [H,W,3] images.
    Identical to fuse() over the back-projected clouds."""
    model = None
    colors = iter(colors) if colors is not None else None
    for depth in depth_images:
        col = next(colors) if colors is not None else None
        if depth is None or not np.any(depth):
            if verbose:
                print("No valid point cloud captured, skipping frame.")      # main.py:53-54
            continue
        if model is None:
            model = cloud_ops.ResidentModel(ctx)
            if model.append_depth(depth, camera, col) == 0:
                model.close()
                model = None
            continue
        res = model.align_append_depth(depth, camera, col, threshold, voxel_size, max_iter, cloud_ops.P2P, 2 * voxel_size, 30)
        if res["frame_points"] == 0:                                          # nothing within depth_trunc: a failed capture
            continue
        if log is not None:
            log.append(res)
    if model is None:
        return PointCloud()
    pts, cols, nrm = model.download()
    if log is not None:
        v, r, u = model.voxel_table_stats()
        log_stats = {"voxel_table": {"voxels": v, "rebuilds": r, "updates": u}}
        if log:
            log[-1].update(log_stats)
    model.close()
    return PointCloud(pts, cols, nrm)


def _fuse_host(frames, flavour, verbose, log, **align_kw):
    model = PointCloud()
    aligner = PointCloudAlignment(verbose=verbose) if flavour == "icp" else GeneralizedICPAlignment()
    for frame in frames:
        if frame is None or len(as_arrays(frame)[0]) == 0:
            if verbose:
                print("No valid point cloud captured, skipping frame.")      # main.py:53-54
            continue
        p, c, n = as_arrays(frame)
        if len(model.points) == 0:
            model.points = p.copy()                                          # main.py:42-45: points + colors only
            model.colors = c.copy() if c is not None else np.zeros((0, 3))
            if flavour == "gicp" and n is not None:
                model.normals = n.copy()
            continue
        aligned = aligner.align_point_clouds(frame, model, **align_kw)
        if log is not None:
            log.append(aligner.last_result)
        model += aligned                                                     # main.py:49
        if flavour == "gicp":                                                # GICP1.py:148: re-estimate on the model
            model.estimate_normals(radius=0.05, max_nn=30)
    return model


def scaled_Q(Q, scale, unit=1.0):
    """Q of the 960x540 rig (tests/golden/jetson_stereo_8MP_stereo.npz) re-expressed for images `scale` times larger.
    The rig was calibrated in millimetres (baseline 31.5): unit=1e-3 yields metres, the unit of the scanner half."""
    Q = np.array(Q, dtype=np.float64)
    Q[0, 3] *= scale
    Q[1, 3] *= scale
    Q[2, 3] *= scale
    Q[:3] *= unit
    return Q


def _color_image(color, left, H, W):
    """The image a view's cloud is coloured from: `left` itself (color=True) or a uint8 [H,W] / [H,W,3] array of the pair's size."""
    img = left if color is True else np.asarray(color)
    if img.dtype != np.uint8 or img.shape[:2] != (H, W) or not (img.ndim == 2 or (img.ndim == 3 and img.shape[2] == 3)):
        raise ValueError(f"color: expected a uint8 image [{H},{W}] or [{H},{W},3], got {img.dtype} {tuple(img.shape)}")
    return np.ascontiguousarray(img)


def view_to_cloud(left, right, Q, matcher, voxel=0.01, normal_radius=None, max_nn=30, pose=None, max_depth=None,
                  device_resident=True, color=None, color_order="bgr"):
    """One stereo view -> down-sampled cloud with normals.  pose (4x4, optional) is applied to the cloud.  left / right: uint8
    [H,W] or [H,W,3] (BGR pairs, as the matcher takes them).
    device_resident (default): the disparity map never leaves HBM; the matcher writes it with compute_device and
    r3d_disparity_to_cloud_dev chains reprojection, depth filter, pose, voxel grid and normals on the device, so only the
    two input images go up and the final cloud comes down.  False: the same stages through the host-buffer entry points
    (identical results; kept for callers that want the intermediate arrays).
    color: None (no colours, as before), True (colour the cloud from `left`) or a uint8 [H,W] / [H,W,3] image of the pair's
    size (e.g. the rectified BGR frame of a grey pair); color_order "bgr" (cv2) or "rgb" says how a 3-channel image is stored.
    The cloud's .colors are r, g, b in [0, 1]; a voxel's colour is the mean over its members."""
    if color_order not in ("bgr", "rgb"):
        raise ValueError(f"color_order must be 'bgr' or 'rgb', got {color_order!r}")
    L = np.ascontiguousarray(left, dtype=np.uint8)
    R = np.ascontiguousarray(right, dtype=np.uint8)
    H, W = L.shape[:2]
    cn = 1 if L.ndim == 2 else L.shape[2]
    img = None if color is None else _color_image(color, L, H, W)
    if device_resident:
        ctx = matcher.context
        d_l, d_r, d_d = ctx.to_device(L), ctx.to_device(R), ctx.alloc(W * H * 2)
        d_c = None
        try:
            matcher.compute_device(d_l, d_r, W, H, W * cn, d_d, channels=cn)
            ckw = {}
            if img is not None:
                d_c = d_l if img is L else ctx.to_device(img)
                ckw = dict(d_color=d_c, color_channels=1 if img.ndim == 2 else 3, color_order=color_order)
            res = cloud_ops.disparity_to_cloud_device(d_d, W, H, Q, matcher.getMinDisparity(), max_depth, pose, voxel,
                                                      normal_radius or 2 * voxel, max_nn, ctx=ctx, **ckw)
        finally:
            for p in (d_l, d_r, d_d) + ((d_c,) if d_c is not None and d_c != d_l else ()):
                ctx.free(p)
        if not len(res[0]):
            return PointCloud()
        return PointCloud(res[0], res[2] if img is not None else None, res[1])
    disp = matcher.compute(L, R)
    pts, pix = cloud_ops.reproject_disparity(disp, Q, matcher.getMinDisparity(), want_pixels=True)
    if len(pts):                                       # zero disparities reproject to infinity (W = 0): never part of a cloud
        keep = np.abs(pts[:, 2]) <= (max_depth if max_depth is not None else 1.0e300)
        pts, pix = pts[keep], pix[keep]
    if len(pts) == 0:
        return PointCloud()
    cols = None
    if img is not None:
        cols = img.reshape(H * W, -1)[pix] / 255.0
        cols = np.repeat(cols, 3, 1) if cols.shape[1] == 1 else (cols[:, ::-1] if color_order == "bgr" else cols)
    if pose is not None:
        pts = cloud_ops.transform_points(pts, pose)
    pts, cols, _ = cloud_ops.voxel_down_sample(pts, voxel, colors=cols)
    nrm = cloud_ops.estimate_normals(pts, normal_radius or 2 * voxel, max_nn)
    return PointCloud(pts, cols, nrm)


def _color_out(out, d_color):
    """Where the colours of a device-tensor view chain go: plane 2 of a [3, capacity, 3] `out` (None without a colour image)."""
    if d_color is None:
        return None
    if out.dim() != 3 or out.shape[0] != 3 or out.shape[2] != 3:
        raise ValueError(f"out: with d_color a [3, capacity, 3] tensor is needed (plane 2 receives the colours), got {tuple(out.shape)}")
    return out[2].data_ptr()


def view_to_cloud_tensors(d_left, d_right, d_disp, width, height, Q, matcher, out, voxel=0.01, normal_radius=None, max_nn=30,
                          pose=None, max_depth=None, d_color=None, color_stride=None, color_channels=3, color_order="bgr"):
    """One stereo view whose images are already in HBM -> cloud left in HBM.  d_left / d_right / d_disp: device pointers
    (uint8 images, int16 disparity scratch); out: float64 torch tensor [2, capacity, 3] on the matcher's device that receives
    points (plane 0) and normals (plane 1).  Returns the tensor view out[:, :n] ([2, n, 3]).  Nothing crosses PCIe but the
    point count.  The library kernels are ordered with torch's current stream (distributed.shared_stream): whatever torch
    queued on the inputs before the call is seen, and torch ops / collectives queued on `out` afterwards see the cloud.
    d_color (device pointer of a uint8 image of the map's size; color_stride / color_channels / color_order as in
    cloud_ops.disparity_to_cloud_device): `out` must then be [3, capacity, 3] and plane 2 receives the colours.  The matched
    images d_left / d_right are one-channel with rows `width` bytes apart; only d_color may have three channels."""
    ctx = matcher.context
    d_out_colors = _color_out(out, d_color)
    with distributed.shared_stream(ctx):
        matcher.compute_device(d_left, d_right, width, height, width, d_disp)
        cap = out.shape[1]
        n = cloud_ops.disparity_to_cloud_resident(d_disp, width, height, Q, out[0].data_ptr(), out[1].data_ptr(), cap,
                                                  matcher.getMinDisparity(), max_depth, pose, voxel, normal_radius or 2 * voxel,
                                                  max_nn, ctx=ctx, d_color=d_color, color_stride=color_stride,
                                                  color_channels=color_channels, color_order=color_order, d_out_colors=d_out_colors)
    return out[:, :n]


def views_to_cloud_tensors(pairs, d_disps, width, height, Q, matcher, outs, cloud_ctx, voxel=0.01, normal_radius=None, max_nn=30,
                           poses=None, max_depth=None, d_colors=None, color_stride=None, color_channels=3, color_order="bgr"):
    """Several views owned by ONE GPU (a rank that holds more than one view of the C5 batch): the same results as one
    view_to_cloud_tensors call per view, but the SGM maps go through the matcher's batch entry point (three maps in flight on
    the library's lanes, r3d_sgbm_compute_batch_events_dev) and the cloud stages of view i (reprojection -> voxel grid ->
    normals) start on map i's completion event, underneath the SGM kernels of the later views, on `cloud_ctx`: a second Context
    with its own stream and arena, or a LIST of them -- the cloud stages are a chain of small kernels with host round trips in
    between, so each extra context gets its own host thread (ctypes releases the GIL) and the chains of different views overlap.
    pairs: [(d_left, d_right)] device pointers; d_disps: one int16 device buffer PER view; outs: one [2, capacity, 3] float64
    tensor per view.  Returns [out_i[:, :n_i]].
    d_colors: one device uint8 image per view (color_stride / color_channels / color_order as in view_to_cloud_tensors); every
    outs[i] must then be [3, capacity, 3] and its plane 2 receives the colours.  The matched pairs are one-channel images with
    rows `width` bytes apart; only the colour images may have three channels."""
    import torch
    ctx = matcher.context
    n = len(pairs)
    cctxs = list(cloud_ctx) if isinstance(cloud_ctx, (list, tuple)) else [cloud_ctx]
    if d_colors is not None and len(d_colors) != n:
        raise ValueError(f"d_colors: {len(d_colors)} images for {n} views")
    d_cols = list(d_colors) if d_colors is not None else [None] * n
    d_out_cols = [_color_out(o, c) for o, c in zip(outs, d_cols)]
    assert len(d_disps) == n and len(outs) == n and all(c is not ctx for c in cctxs) and len({id(c) for c in cctxs}) == len(cctxs)
    dev = outs[0].device
    evs = [ctx.event() for _ in range(n)]
    res = [None] * n
    try:
        with distributed.shared_stream(ctx) as sa:
            import os
            prio = -1 if os.environ.get("R3D_CLOUD_PRIO") == "1" else 0
            sbs = [torch.cuda.Stream(device=dev, priority=prio) for _ in cctxs]
            prev = [c.get_stream() for c in cctxs]
            for c, sb, pv in zip(cctxs, sbs, prev):
                sb.wait_stream(sa)
                if pv:        # work the cloud context queued earlier on its previous stream (it reuses the same arena) stays ahead
                    sb.wait_stream(torch.cuda.ExternalStream(pv, device=dev))
                c.set_stream(sb.cuda_stream)
            try:
                matcher.compute_batch_device([p[0] for p in pairs], [p[1] for p in pairs], width, height, width, list(d_disps),
                                             done_events=evs)

                def chain(w):
                    c = cctxs[w]
                    for i in range(w, n, len(cctxs)):
                        c.wait_event(evs[i])
                        k = cloud_ops.disparity_to_cloud_resident(d_disps[i], width, height, Q, outs[i][0].data_ptr(), outs[i][1].data_ptr(),
                                                                  outs[i].shape[1], matcher.getMinDisparity(), max_depth,
                                                                  None if poses is None else poses[i], voxel, normal_radius or 2 * voxel,
                                                                  max_nn, ctx=c, d_color=d_cols[i], color_stride=color_stride,
                                                                  color_channels=color_channels, color_order=color_order,
                                                                  d_out_colors=d_out_cols[i])
                        res[i] = outs[i][:, :k]
                if len(cctxs) == 1:
                    chain(0)
                else:
                    from concurrent.futures import ThreadPoolExecutor
                    with ThreadPoolExecutor(len(cctxs)) as pool:
                        for f in [pool.submit(chain, w) for w in range(len(cctxs))]:
                            f.result()                       # re-raises a worker's exception here
            finally:
                # on EVERY path (a worker may have raised with the other chains' kernels still queued): the matcher's stream joins
                # the side streams, so that the ctx.sync() below also covers kernels that write outs[i] / read d_disps[i]
                for sb in sbs:
                    sa.wait_stream(sb)
                for c, p in zip(cctxs, prev):
                    c.set_stream(p)
    finally:
        ctx.sync()
        for e in evs:
            ctx.call("r3d_event_destroy", ctypes.c_void_p(e))
    return res


def multi_view_fuse_tensors(local, n_views, threshold=0.02, mode=cloud_ops.GICP, max_iteration=30, register=None, transform=None,
                            ctx=None, timings=None):
    """BASELINE config C5 on clouds that live where the exchange runs (HBM under RCCL).  local: {view_id: float64 tensor
    [2, n, 3]} (points, normals) of the views this rank owns (distributed.shard_views).  Steps: ONE all-gather-v of the clouds
    (distributed.gather_views) -> every owned view is registered to view 0 (r3d_icp_dev on the gathered blocks, in place) ->
    the 4x4s are all-gathered -> every view is transformed into the frame of view 0 (r3d_transform_blocks_dev: one launch) into one fused
    [2, N, 3] tensor, which every rank ends up holding (rank 0 hands it to the mesher, mesh_reconstruction.py:22-37).
    Returns (fused tensor, {view_id: T}).  `register(src [2,n,3], tgt [2,m,3]) -> 4x4` and `transform(block, T) -> block`
    replace the HIP calls in the CPU (gloo) tests; with device tensors and no stubs the HIP library does the work.
    Views may carry a third plane, colours ([3, n, 3], pipeline.view_to_cloud_tensors with d_color): it travels through the same
    all-gather and is copied unchanged into a fused [3, N, 3] tensor (the stubs still see and return planes 0 and 1 only).  All
    views must have the same number of planes: ValueError otherwise, on every rank, before the first collective.
    mode=cloud_ops.COLORED registers every view to view 0 with the coloured registration (r3d_icp_colored_dev on planes 0 / 1 / 2:
    source points and colours, target points, normals and colours); it needs three-plane views (ValueError on every rank, before
    the payload exchange, otherwise) and the `register` stub then receives all three planes of both views.
    timings (dict, optional) receives exchange_ms / register_ms / fuse_ms measured with events on the shared stream.
    (A rank that owns several views registers them one after the other: running them on several contexts / host threads at
    once was measured -- 7 registrations of 109 k-point clouds: 2.8 ms sequential, 3.3-3.8 ms on two contexts, 2.5-3.0 ms on
    four -- and dropped.)"""
    import torch
    dev = distributed.exchange_device()
    on_gpu = dev.type == "cuda"
    if not on_gpu and (register is None or transform is None):
        raise RuntimeError("multi_view_fuse_tensors: host tensors need injected register / transform stubs; the product path "
                           "runs on device tensors through libr3d_hip.so (no CPU fallback)")
    if on_gpu and ctx is None:
        from . import _lib
        ctx = _lib.default_context(dev.index or 0)
    if on_gpu:
        # ONE stream for torch ops, RCCL collectives and library kernels for the whole exchange (the context's own
        # stream is not ordered against torch's)
        outer = torch.cuda.current_stream(dev)
        with distributed.shared_stream(ctx):
            fused, Ts = _multi_view_fuse_on_stream(local, n_views, threshold, mode, max_iteration, register, transform, ctx, timings, dev)
        fused.record_stream(outer)
        return fused, Ts
    return _multi_view_fuse_on_stream(local, n_views, threshold, mode, max_iteration, register, transform, ctx, timings, dev)


def _multi_view_fuse_on_stream(local, n_views, threshold, mode, max_iteration, register, transform, ctx, timings, dev):
    import torch
    on_gpu = dev.type == "cuda"

    def mark():
        if not on_gpu:
            import time
            return time.perf_counter()
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        return e

    def lap(a, b):
        if not on_gpu:
            return 1e3 * (b - a)
        b.synchronize()
        return a.elapsed_time(b)

    planes = distributed.common_planes(local)            # 2, or 3 with colours; raises on every rank if the views disagree
    colored = mode == cloud_ops.COLORED
    if colored and planes != 3:
        # the count is the one all ranks agreed on, so every rank raises here, before the payload exchange
        raise ValueError("mode=COLORED registers on the views' colours: every view must be a [3, n, 3] tensor (points, normals, colours)")
    t0 = mark()
    everyone = distributed.gather_views(local, n_views, planes=planes)
    t1 = mark()
    ref = everyone[0]
    mine = {}

    def register_view(v, c):
        # a registration that fails on this rank must not strand the others in the next collective: the exception travels as
        # a flag through gather_transforms, which then raises on every rank together
        try:
            if v == 0:
                return np.eye(4)
            if register is not None:
                if colored:
                    return np.asarray(register(everyone[v], ref), dtype=np.float64)
                return np.asarray(register(everyone[v][:2], ref[:2]), dtype=np.float64)
            src = everyone[v]
            if colored:
                return cloud_ops.registration_colored_device(src[0].data_ptr(), src[2].data_ptr(), src.shape[1], ref[0].data_ptr(),
                                                             ref[1].data_ptr(), ref[2].data_ptr(), ref.shape[1], threshold,
                                                             max_iteration=max_iteration, ctx=c)["T"]
            return cloud_ops.registration_device(src[0].data_ptr(), src.shape[1], ref[0].data_ptr(), ref.shape[1], threshold,
                                                 mode=mode, max_iteration=max_iteration, d_source_normals=src[1].data_ptr(),
                                                 d_target_normals=ref[1].data_ptr(), ctx=c)["T"]
        except Exception as e:  # noqa: BLE001
            return e
    for v in local:
        mine[v] = register_view(v, ctx)
    t2 = mark()
    Ts = distributed.gather_transforms(mine, n_views)
    total = sum(everyone[v].shape[1] for v in range(n_views))
    fused = torch.empty((planes, total, 3), dtype=torch.float64, device=dev)
    o = 0
    blocks = []
    for v in range(n_views):
        blk, n = everyone[v], everyone[v].shape[1]
        if planes == 3:
            fused[2, o:o + n] = blk[2]                 # colours: no rigid transform touches them
        if transform is not None:
            fused[:2, o:o + n] = transform(blk[:2], Ts[v])
        elif n:
            blocks.append((blk[0].data_ptr(), n, Ts[v], fused[0, o:o + n].data_ptr(), False))
            blocks.append((blk[1].data_ptr(), n, Ts[v], fused[1, o:o + n].data_ptr(), True))
        o += n
    if blocks:       # points and normals of all views in ONE launch (sixteen calls cost 0.3 ms of host overhead, profiles/r03_bench.json)
        cloud_ops.transform_blocks_device(blocks, ctx=ctx)
    t3 = mark()
    if timings is not None:
        timings.update(exchange_ms=lap(t0, t1), register_ms=lap(t1, t2), fuse_ms=lap(t2, t3))
    return fused, Ts


def multi_view_fuse(local_clouds, n_views, threshold=0.02, mode=cloud_ops.GICP, max_iteration=30, register=None, ctx=None):
    """Host-cloud front end of multi_view_fuse_tensors.  local_clouds: {view_id: PointCloud with normals} owned by this rank.
    The clouds go up once (to the device the exchange runs on), everything else stays there; returns
    (fused PointCloud, {view_id: T}).  `register(src [n,6], tgt [m,6]) -> 4x4` may replace the HIP registration (the CPU tests
    inject a stub; rows are xyz | normal, and xyz | normal | rgb with mode=cloud_ops.COLORED, which needs colours on every
    view).  Clouds with colours keep them: the colours ride along as a third plane and the fused
    cloud has .colors; colours on some views only (on any rank) raise ValueError."""
    import torch
    dev = distributed.exchange_device()
    local = {}
    for v, pc in local_clouds.items():
        p, c, n = as_arrays(pc)
        planes = [p, n if n is not None else np.zeros_like(p)] + ([c] if c is not None else [])
        local[v] = torch.from_numpy(np.stack(planes, 0)).to(dev)
    reg = tr = None
    if register is not None:
        def reg(src, tgt):      # rows xyz | normal, and | rgb behind them in the coloured mode (the only one that hands colours over)
            return register(torch.cat(list(src), 1).cpu().numpy(), torch.cat(list(tgt), 1).cpu().numpy())
    if dev.type != "cuda" or register is not None:
        def tr(blk, T):
            R = torch.from_numpy(np.ascontiguousarray(T[:3, :3])).to(blk.device)
            t = torch.from_numpy(np.ascontiguousarray(T[:3, 3])).to(blk.device)
            return torch.stack([blk[0] @ R.T + t, blk[1] @ R.T], 0)
    fused, Ts = multi_view_fuse_tensors(local, n_views, threshold, mode, max_iteration, reg, tr, ctx)
    arr = fused.cpu().numpy()
    return PointCloud(arr[0], arr[2] if len(arr) == 3 else None, arr[1]), Ts


def odometry_edges(frames, camera, ctx=None, **option):
    """The pose-graph edges of consecutive frames (test/check84.py:236-255): frame i+1 -> frame i by RGB-D odometry from the
    identity.  frames: (colour uint8 [H,W,3] or [H,W], depth uint16 [H,W]) pairs or cloud_ops.RGBDImage; camera:
    cloud_ops.depth_camera(...), whose depth_scale and depth_trunc read the raw pairs.  A failed pair gives the identity and
    uncertain=True, as the script's fallback edge.  -> [dict(source, target, T, info, uncertain)]"""
    imgs = [f if isinstance(f, cloud_ops.RGBDImage) else cloud_ops.rgbd_image(f[0], f[1], camera.depth_scale, camera.depth_trunc) for f in frames]
    edges = []
    for i in range(len(imgs) - 1):
        ok, T, info = cloud_ops.compute_rgbd_odometry(imgs[i + 1], imgs[i], camera, ctx=ctx, **option)
        edges.append(dict(source=i + 1, target=i, T=T if ok else np.eye(4), info=info if ok else np.eye(6), uncertain=not ok))
    return edges


def poses_from_edges(edges):
    """Camera-to-world poses of the frames from a chain of pairwise edges, the first frame being the world: the composition of
    test/check84.py's loop, odometry = T @ odometry, node pose = inv(odometry), where T takes frame k to frame k + 1.  An edge
    of odometry_edges runs the other way (source k + 1 -> target k), so its T enters inverted; an edge with source k and
    target k + 1 enters as it is.  -> [4x4] of len(edges) + 1"""
    odometry = np.eye(4)
    poses = [np.eye(4)]
    for k, e in enumerate(edges):
        T = np.asarray(e["T"], dtype=np.float64).reshape(4, 4)
        if (e["source"], e["target"]) == (k + 1, k):
            T = np.linalg.inv(T)
        elif (e["source"], e["target"]) != (k, k + 1):
            raise ValueError(f"edge {k} joins frames {e['source']} -> {e['target']}: poses_from_edges composes a chain of consecutive frames")
        odometry = T @ odometry
        poses.append(np.linalg.inv(odometry))
    return poses


def loop_closure_edges(frames, camera, every, ctx=None, **option):
    """The loop-closure candidates of Open3D's make_fragments rule: RGB-D odometry from the identity between frames s < t with
    s % every == 0, t % every == 0 and t - s > 1, source t -> target s (the direction of odometry_edges), uncertain=True.  A failed
    pair is left out.  frames, camera, option: as odometry_edges.  -> [dict(source, target, T, info, uncertain)]"""
    every = int(every)
    if every < 1:
        raise ValueError(f"every={every}: a positive key-frame distance is needed")
    imgs = [f if isinstance(f, cloud_ops.RGBDImage) else cloud_ops.rgbd_image(f[0], f[1], camera.depth_scale, camera.depth_trunc) for f in frames]
    edges = []
    for s in range(0, len(imgs), every):
        for t in range(s + every, len(imgs), every):
            if t - s <= 1:
                continue
            ok, T, info = cloud_ops.compute_rgbd_odometry(imgs[t], imgs[s], camera, ctx=ctx, **option)
            if ok:
                edges.append(dict(source=t, target=s, T=T, info=info, uncertain=True))
    return edges


def pose_graph_from_edges(edges, poses=None):
    """A posegraph.PoseGraph of edge dicts (odometry_edges, loop_closure_edges): the node poses are poses_from_edges(edges) when
    the edges are a chain of consecutive frames, otherwise `poses` (camera-to-world 4x4 per frame), which must then be given."""
    from . import posegraph
    if poses is None:
        poses = poses_from_edges(edges)
    nodes = [posegraph.PoseGraphNode(p) for p in poses]
    return posegraph.PoseGraph(nodes, [posegraph.PoseGraphEdge(e["source"], e["target"], e["T"], e["info"], e["uncertain"], e.get("confidence", 1.0))
                                       for e in edges])


def optimize_poses(edges, loop_closures=(), poses=None, criteria=None, option=None, ctx=None):
    """test/check84.py:262-273: the poses of the frames after global_optimization of the graph of `edges` (a chain, odometry_edges)
    and `loop_closures` (loop_closure_edges).  poses: the initial node poses; default poses_from_edges(edges).  option: default
    GlobalOptimizationOption(reference_node=0), as the script's.  -> [4x4], which tsdf_fuse takes"""
    from . import posegraph
    graph = pose_graph_from_edges(list(edges) + list(loop_closures), poses if poses is not None else poses_from_edges(edges))
    posegraph.global_optimization(graph, posegraph.GlobalOptimizationLevenbergMarquardt(), criteria,
                                  option or posegraph.GlobalOptimizationOption(reference_node=0), ctx=ctx)
    return [n.pose for n in graph.nodes]


def mesh_postprocess(mesh, smooth_iterations=5, lambda_filter=0.5, ctx=None, min_component_triangles=0, keep_largest_component=False, weld=False):
    """The tail of mesh_reconstruction.py:22-37 after its Poisson call, restricted to what this package has, in the order of
    SURVEY.md section 2: filter_smooth_laplacian(smooth_iterations), remove_degenerate_triangles, remove_unreferenced_vertices and
    the non-finite scrub of check84.py:315-322, then compute_vertex_normals.  ASSUMED (the reference source is not in this
    repository): lambda 0.5 and FilterScope.All, Open3D's defaults.  The non-finite vertices go before the unreferenced ones, so
    that a vertex left without triangles by the scrub goes too.  The topology clean-ups are off by default (the marching-cubes mesh
    has no duplicates to remove, and today's output stays bit for bit); they run after the scrubs and before the normals:
    weld=True: remove_duplicated_vertices and remove_duplicated_triangles; min_component_triangles / keep_largest_component:
    remove_small_components.  remove_non_manifold_edges is not built.  -> a new TriangleMesh"""
    out = mesh.filter_smooth_laplacian(int(smooth_iterations), lambda_filter, ctx=ctx)
    out.remove_degenerate_triangles(ctx=ctx).remove_non_finite_vertices(ctx=ctx).remove_unreferenced_vertices(ctx=ctx)
    if weld:
        out.remove_duplicated_vertices(ctx=ctx).remove_duplicated_triangles(ctx=ctx)
    if min_component_triangles > 0 or keep_largest_component:
        out.remove_small_components(min_triangles=int(min_component_triangles), keep_largest=bool(keep_largest_component), ctx=ctx)
    return out.compute_vertex_normals(device=True, ctx=ctx)


def reconstruct_mesh(cloud, depth=6, smooth_iterations=5, ctx=None):
    """mesh_reconstruction.py:22-37 from its first line: create_from_point_cloud_poisson(depth) of a cloud with normals (and
    colours), then mesh_postprocess(smooth_iterations).  -> TriangleMesh"""
    from . import poisson
    mesh, _ = poisson.create_from_point_cloud_poisson(cloud, depth=depth, ctx=ctx)
    return mesh_postprocess(mesh, smooth_iterations, ctx=ctx)


def tsdf_fuse(frames, camera, poses, voxel_length, sdf_trunc, color=True, ctx=None, mesh=False, postprocess=False, postprocess_options=None, **volume_options):
    """test/check84.py:41-44,295,307: every frame into a ScalableTSDFVolume with extrinsic = inv(pose), then
    extract_point_cloud().  frames: (colour, depth uint16) pairs or cloud_ops.RGBDImage, as odometry_edges takes them; camera:
    cloud_ops.depth_camera(...); poses: camera-to-world 4x4 per frame (poses_from_edges).  -> PointCloud with normals[, colours];
    mesh=True: extract_triangle_mesh() instead -> TriangleMesh; postprocess=True (with mesh=True): mesh_postprocess() of it, with the
    keywords of the dict postprocess_options (weld, min_component_triangles, ...)"""
    if len(poses) != len(frames):
        raise ValueError(f"{len(frames)} frames but {len(poses)} poses")
    if postprocess and not mesh:
        raise ValueError("postprocess=True needs mesh=True")
    imgs = [f if isinstance(f, cloud_ops.RGBDImage) else cloud_ops.rgbd_image(f[0], f[1], camera.depth_scale, camera.depth_trunc) for f in frames]
    kind = tsdf.TSDFVolumeColorType.RGB8 if color else tsdf.TSDFVolumeColorType.NoColor
    with tsdf.ScalableTSDFVolume(voxel_length, sdf_trunc, kind, ctx=ctx, **volume_options) as volume:
        for img, pose in zip(imgs, poses):
            volume.integrate(img, camera, np.linalg.inv(np.asarray(pose, dtype=np.float64).reshape(4, 4)))
        if not mesh:
            return volume.extract_point_cloud()
        out = volume.extract_triangle_mesh()
    return mesh_postprocess(out, ctx=ctx, **(postprocess_options or {})) if postprocess else out
