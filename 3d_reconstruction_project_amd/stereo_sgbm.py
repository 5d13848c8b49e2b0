"""Drop-in for the cv2.StereoSGBM object protocol the reference's depth viewers use.

Reference surface (Calib_depth/depth1.py:202-214,240-265,331; depth2.py:146-158,251):
    matcher = cv2.StereoSGBM_create(minDisparity=..., numDisparities=..., blockSize=..., P1=..., P2=...,
                                    disp12MaxDiff=..., uniquenessRatio=..., speckleWindowSize=..., speckleRange=...,
                                    preFilterCap=..., mode=cv2.STEREO_SGBM_MODE_SGBM_3WAY)
    disp = matcher.compute(gray_left, gray_right)        # int16 [H,W], disparity x16, invalid = (minD-1)*16
    disp = matcher.compute(bgr_left, bgr_right)          # cv2 takes CV_8UC3 pairs too: the pixel cost is summed over the channels
    matcher.setBlockSize(b); matcher.getNumDisparities(); ...
Same keyword names, defaults, getters/setters and error behaviour (an exception on bad input).  All arithmetic
runs in the HIP library (csrc/sgm.hip) through the C ABI in include/r3d.h.
"""
import ctypes
import os

import numpy as np

from . import _lib

STEREO_SGBM_MODE_SGBM = 0
STEREO_SGBM_MODE_HH = 1
STEREO_SGBM_MODE_SGBM_3WAY = 2
STEREO_SGBM_MODE_HH4 = 3

_FIELDS = ("minDisparity", "numDisparities", "blockSize", "P1", "P2", "disp12MaxDiff", "preFilterCap",
           "uniquenessRatio", "speckleWindowSize", "speckleRange", "mode")


class StereoSGBM:
    def __init__(self, minDisparity=0, numDisparities=16, blockSize=3, P1=0, P2=0, disp12MaxDiff=0, preFilterCap=0,
                 uniquenessRatio=0, speckleWindowSize=0, speckleRange=0, mode=STEREO_SGBM_MODE_SGBM_3WAY, device=0):
        self._p = dict(minDisparity=minDisparity, numDisparities=numDisparities, blockSize=blockSize, P1=P1, P2=P2,
                       disp12MaxDiff=disp12MaxDiff, preFilterCap=preFilterCap, uniquenessRatio=uniquenessRatio,
                       speckleWindowSize=speckleWindowSize, speckleRange=speckleRange, mode=mode)
        self._device = _lib.parse_device(device)
        self._ctx = None

    # cv2-style accessors (depth1.py:240-265 tunes blockSize / numDisparities from key presses)
    def __getattr__(self, name):
        for pre in ("get", "set"):
            if name.startswith(pre):
                key = name[3:]
                key = key[0].lower() + key[1:]
                if key == "mode":
                    key = "mode"
                if key in self._p or key in ("p1", "p2"):
                    key = {"p1": "P1", "p2": "P2"}.get(key, key)
                    if pre == "get":
                        return lambda: self._p[key]
                    return lambda v: self._p.__setitem__(key, int(v))
        raise AttributeError(name)

    @property
    def context(self):
        if self._ctx is None:
            self._ctx = _lib.default_context(self._device)
        return self._ctx

    def params_struct(self):
        return _lib.SgbmParams(*[int(self._p[k]) for k in _FIELDS])

    @staticmethod
    def _pair(left, right):
        """The two images of a pair as contiguous uint8 arrays and their channel count: both [H,W] (1) or both [H,W,3] (3)."""
        left = np.asarray(left)
        right = np.asarray(right)
        if (left.dtype != np.uint8 or right.dtype != np.uint8 or left.shape != right.shape
                or not (left.ndim == 2 or (left.ndim == 3 and left.shape[2] == 3))):
            raise ValueError("StereoSGBM.compute expects two uint8 images of equal size and kind, both single-channel [H,W] "
                             "or both 3-channel [H,W,3] (cv2's CV_8UC1 / CV_8UC3)")
        return np.ascontiguousarray(left), np.ascontiguousarray(right), 1 if left.ndim == 2 else 3

    def compute(self, left, right):
        """left, right: uint8 rectified images, both grey [H,W] or both colour [H,W,3] (any channel order: the pixel cost is
        the sum over the channels).  Returns int16 [H,W]."""
        left, right, cn = self._pair(left, right)
        H, W = left.shape[:2]
        self._last_shape = (H, W)
        disp = np.empty((H, W), np.int16)
        p = self.params_struct()
        vp = ctypes.c_void_p
        self.context.call("r3d_sgbm_compute_cn", ctypes.byref(p), left.ctypes.data_as(vp), right.ctypes.data_as(vp),
                          W, H, W * cn, cn, disp.ctypes.data_as(vp))
        return disp

    def compute_device(self, d_left, d_right, width, height, stride, d_disp, channels=1):
        """Device-pointer variant (ints): enqueues on the context stream, no synchronisation.  channels: 1, or 3 for
        interleaved colour images (stride in bytes per row, >= width * channels)."""
        p = self.params_struct()
        vp = ctypes.c_void_p
        self.context.call("r3d_sgbm_compute_cn_dev", ctypes.byref(p), vp(d_left), vp(d_right), int(width), int(height),
                          int(stride), int(channels), vp(d_disp))

    def compute_batch_device(self, d_lefts, d_rights, width, height, stride, d_disps, done_events=None, channels=1):
        """Device-pointer batch (lists of ints): maps are pipelined over the library's internal lanes.  done_events (list of
        Context.event() handles or None entries): map i's completion is recorded into done_events[i], so a consumer on another
        context can wait for it (Context.wait_event) while later maps are still running.  channels: as compute_device."""
        n = len(d_lefts)
        assert len(d_rights) == n and len(d_disps) == n and (done_events is None or len(done_events) == n)
        if n > 1:   # three lanes + the context stream (+ the consumers' streams): more than HIP's default four hardware queues
            _lib.warn_if_few_hw_queues(int(os.environ.get("R3D_SGM_LANES", "3")) + 2)
        arr = ctypes.c_void_p * n
        p = self.params_struct()
        if channels != 1:
            self.context.call("r3d_sgbm_compute_batch_cn_dev", ctypes.byref(p), n, arr(*d_lefts), arr(*d_rights), int(width),
                              int(height), int(stride), int(channels), arr(*d_disps),
                              arr(*done_events) if done_events is not None else None)
        elif done_events is None:
            self.context.call("r3d_sgbm_compute_batch_dev", ctypes.byref(p), n, arr(*d_lefts), arr(*d_rights), int(width),
                              int(height), int(stride), arr(*d_disps))
        else:
            self.context.call("r3d_sgbm_compute_batch_events_dev", ctypes.byref(p), n, arr(*d_lefts), arr(*d_rights), int(width),
                              int(height), int(stride), arr(*d_disps), arr(*done_events))

    def compute_batch(self, lefts, rights):
        """lefts / rights: sequences of uint8 images of equal size and kind ([H,W] or [H,W,3]) -> list of int16 disparity maps."""
        ctx = self.context
        shape = np.asarray(lefts[0]).shape
        if not (len(shape) == 2 or (len(shape) == 3 and shape[2] == 3)):
            raise ValueError(f"StereoSGBM.compute_batch expects [H,W] or [H,W,3] images, got shape {shape}")
        if any(np.asarray(a).shape != shape for a in list(lefts) + list(rights)):
            raise ValueError("StereoSGBM.compute_batch expects images of one size and kind (all [H,W] or all [H,W,3])")
        H, W = shape[:2]
        cn = 1 if len(shape) == 2 else 3
        dl = [ctx.to_device(np.ascontiguousarray(a, dtype=np.uint8)) for a in lefts]
        dr = [ctx.to_device(np.ascontiguousarray(a, dtype=np.uint8)) for a in rights]
        dd = [ctx.alloc(W * H * 2) for _ in lefts]
        try:
            self.compute_batch_device(dl, dr, W, H, W * cn, dd, channels=cn)
            ctx.sync()
            out = []
            for d in dd:
                a = np.empty((H, W), np.int16)
                ctx.d2h(a, d)
                out.append(a)
        finally:
            for q in dl + dr + dd:
                ctx.free(q)
        self._last_shape = (H, W)
        return out

    def debug_fetch(self, want_cost=False, want_hsum=False, want_raw=True):
        """Stage outputs of the last compute (parity tests): dict of int16 arrays.  The cost volume of a colour pair is the
        sum over its channels."""
        ctx = self.context
        D = self._p["numDisparities"]
        minD = self._p["minDisparity"]
        H, W = self._last_shape
        W1 = (W + min(minD, 0)) - max(minD + D, 0)
        dp = next(c for c in (32, 64, 128, 256, 512) if D <= c)   # slots per cost-volume column: the smallest that holds D
        out = {}
        cost = np.empty((H, W1, dp), np.int16) if want_cost else None
        hsum = np.empty((H, W1, dp), np.int16) if want_hsum else None
        raw = np.empty((H, W), np.int16) if want_raw else None
        vp = ctypes.c_void_p
        ctx.call("r3d_sgbm_debug_fetch", cost.ctypes.data_as(vp) if want_cost else None,
                 hsum.ctypes.data_as(vp) if want_hsum else None, raw.ctypes.data_as(vp) if want_raw else None)
        if want_cost:
            out["cost"] = cost[:, :, :D]
        if want_hsum:
            out["hsum"] = hsum[:, :, :D]
        if want_raw:
            out["raw"] = raw
        return out

    def debug_hh_partial(self, n):
        """MODE_HH stage parity: S after the first n directions (1..8, contract order) of the last compute, int16 [H, W1, D].
        The library runs those directions again over the cost volume of that compute; afterwards debug_fetch's hsum is this
        volume, its cost and raw are unchanged."""
        D = self._p["numDisparities"]
        minD = self._p["minDisparity"]
        H, W = self._last_shape
        W1 = max((W + min(minD, 0)) - max(minD + D, 0), 0)
        dp = next((c for c in (32, 64, 128, 256, 512) if D <= c), 512)
        S = np.empty((H, W1, dp), np.int16)
        self.context.call("r3d_sgbm_debug_hh_partial", int(n), S.ctypes.data_as(ctypes.c_void_p))
        return S[:, :, :D]

    def debug_select(self, cost, hsum, cspec=None, cost_pad=0, hsum_pad=32767, width=None):
        """Selection-stage parity: runs the vertical path + winner-take-all (MODE_SGBM_3WAY) or the eighth direction fused with
        the selection (MODE_HH), then the LR check, on the caller's volumes with this matcher's parameters.
        cost, hsum: int16 [H, W1, D] (cost in 0..16383); cspec: optional int16 [3, blockSize // 2, W1, D], the block-cost rows
        stripes 1..3 read for their first rows; cost_pad / hsum_pad fill the volume slots past D, which must not change any
        result.  width: the image width (default: the one whose matching range has W1 columns).
        Returns dict(raw_wta, mins, lrd) of int16 [H, width]."""
        D, minD = self._p["numDisparities"], self._p["minDisparity"]
        cost = np.ascontiguousarray(cost, dtype=np.int16)
        hsum = np.ascontiguousarray(hsum, dtype=np.int16)
        H, W1 = cost.shape[:2]
        W = int(width) if width is not None else W1 + max(minD + D, 0) - min(minD, 0)
        if cost.shape != (H, W1, D) or hsum.shape != cost.shape or (W + min(minD, 0)) - max(minD + D, 0) != W1:
            raise ValueError(f"debug_select expects cost and hsum of shape [H, W1, {D}] with W1 the matching range of width {W}")
        vp = ctypes.c_void_p
        if cspec is not None:
            cspec = np.ascontiguousarray(cspec, dtype=np.int16)
            if cspec.shape != (3, self._p["blockSize"] // 2, W1, D):
                raise ValueError(f"debug_select expects cspec of shape [3, blockSize // 2, W1, D], got {cspec.shape}")
        out = {k: np.empty((H, W), np.int16) for k in ("raw_wta", "mins", "lrd")}
        p = self.params_struct()
        self.context.call("r3d_sgbm_debug_select", ctypes.byref(p), W, H, cost.ctypes.data_as(vp), _opt_ptr(cspec), hsum.ctypes.data_as(vp),
                          int(cost_pad), int(hsum_pad), *[out[k].ctypes.data_as(vp) for k in ("raw_wta", "mins", "lrd")])
        self._last_shape = (H, W)
        return out

    def debug_fetch_select(self):
        """raw_wta (disparity x16 before the LR check), mins (min S) and lrd (after the LR check) of the last compute or
        debug_select: dict of int16 [H, W].  raw_wta and mins are defined at the matching columns only."""
        H, W = self._last_shape
        out = {k: np.empty((H, W), np.int16) for k in ("raw_wta", "mins", "lrd")}
        self.context.call("r3d_sgbm_debug_fetch_select", *[out[k].ctypes.data_as(ctypes.c_void_p) for k in ("raw_wta", "mins", "lrd")])
        return out


def _opt_ptr(a):
    """ctypes pointer of an optional array (None -> NULL)."""
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


def filterSpeckles(img, newVal, maxSpeckleSize, maxDiff, device=0):
    """cv2.filterSpeckles on an int16 image; returns the filtered copy."""
    a = np.ascontiguousarray(img, dtype=np.int16).copy()
    H, W = a.shape
    _lib.default_context(_lib.parse_device(device)).call("r3d_filter_speckles", a.ctypes.data_as(ctypes.c_void_p), W, H,
                                                         int(newVal), int(maxSpeckleSize), int(maxDiff))
    return a


def StereoSGBM_create(minDisparity=0, numDisparities=16, blockSize=3, P1=0, P2=0, disp12MaxDiff=0, preFilterCap=0,
                      uniquenessRatio=0, speckleWindowSize=0, speckleRange=0, mode=STEREO_SGBM_MODE_SGBM, device=0):
    """Factory with cv2.StereoSGBM_create's keyword names and defaults.  MODE_SGBM_3WAY (the mode every reference call
    site passes) and MODE_HH (eight full-image paths, no stripes) are implemented; MODE_SGBM and MODE_HH4 raise at
    compute().  compute() takes grey [H,W] or colour [H,W,3] pairs, as cv2 does.  numDisparities: a multiple of 16 up to 512 (above 256 the cost volumes use 512 slots per column: 1 KB per
    cost column and volume, two volumes per map in flight)."""
    return StereoSGBM(minDisparity, numDisparities, blockSize, P1, P2, disp12MaxDiff, preFilterCap, uniquenessRatio,
                      speckleWindowSize, speckleRange, mode, device)


def createRightMatcher(matcher_left):
    """cv2.ximgproc.createRightMatcher(matcher_left) (Calib_depth/depth1.py:215, depth2.py:161): a StereoSGBM with
    minDisparity = -(minD + D) + 1, the same D / blockSize / P1 / P2 / preFilterCap / mode, uniquenessRatio 0,
    disp12MaxDiff 1000000 and no speckle filter; it is called as compute(right, left) (depth2.py:252)."""
    p = matcher_left._p
    return StereoSGBM(minDisparity=-(p["minDisparity"] + p["numDisparities"]) + 1, numDisparities=p["numDisparities"],
                      blockSize=p["blockSize"], P1=p["P1"], P2=p["P2"], disp12MaxDiff=1000000, preFilterCap=p["preFilterCap"],
                      uniquenessRatio=0, speckleWindowSize=0, speckleRange=0, mode=p["mode"], device=matcher_left._device)


def reference_matcher(numDisparities=128, blockSize=5, family="depth2", device=0):
    """The two parameter families the reference uses (Calib_depth/depth2.py:139-158, depth4.py:147-168)."""
    kw = dict(minDisparity=0, numDisparities=numDisparities, blockSize=blockSize, P1=8 * 3 * blockSize ** 2,
              P2=32 * 3 * blockSize ** 2, disp12MaxDiff=1, preFilterCap=63, mode=STEREO_SGBM_MODE_SGBM_3WAY)
    if family in ("depth1", "depth2", "depth3"):
        kw.update(uniquenessRatio=15, speckleWindowSize=0, speckleRange=2)
    elif family in ("depth4", "depth_test"):
        kw.update(uniquenessRatio=10, speckleWindowSize=50, speckleRange=32)
    else:
        raise ValueError(family)
    return StereoSGBM_create(device=device, **kw)


def depth(left, right, **params):
    """north_star alias: one-shot disparity map with reference (depth2.py) defaults overridable by kwargs."""
    fam = params.pop("family", "depth2")
    m = reference_matcher(params.pop("numDisparities", 128), params.pop("blockSize", 5), fam, params.pop("device", 0))
    for k, v in params.items():
        m._p[k] = int(v)
    return m.compute(left, right)
