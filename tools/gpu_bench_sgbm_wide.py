"""SGBM at 3264x2448 with 256 and with 512 disparities (the reference's depth2 parameters) on the synthetic pair of
synth.stereo_pair, in ONE process: for each D, MODE_SGBM_3WAY and MODE_HH with one map in flight: ms per map (device events,
after warm-up, 10 timed maps) and per-kernel ms (r3d_set_profiling / sgbm_profile over 10 further maps), then every kernel's
D = 512 : D = 256 ratio next to the ratio of the bytes the volumes hold, (W - 512) * 512 : (W - 256) * 256 = 1.83.  The
D = 512 3WAY map is also compared with the C oracle (the whole map, a volume of 6.9 GB).
Usage (GPU box): python tools/gpu_bench_sgbm_wide.py [out.json]   (default: profiles/sgbm_wide_c2.json)"""
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
r3d = importlib.import_module("3d_reconstruction_project_amd")
from oracle import sgbm_oracle as so  # noqa: E402

W, H = 3264, 2448
KW = dict(minDisparity=0, blockSize=5, P1=600, P2=2400, disp12MaxDiff=1, uniquenessRatio=15, speckleWindowSize=0,
          speckleRange=2, preFilterCap=63)           # Calib_depth/depth2.py:146-158
WARMUP, MAPS = 3, 10
VOLUME_KERNELS = {"3way": ("cost", "hscan", "vscan_wta"),
                  "hh": ("cost", "hh_right", "hh_down_right", "hh_down", "hh_down_left", "hh_left", "hh_up_right", "hh_up", "hh_up_left_wta")}


def volume_bytes(D):
    dp = next(c for c in (32, 64, 128, 256, 512) if D <= c)
    return (W - D) * H * dp * 2


def measure(m, ctx, bufs):
    d_l, d_r, d_d = bufs
    e0, e1 = ctx.event(), ctx.event()
    for _ in range(WARMUP):
        m.compute_device(d_l, d_r, W, H, W, d_d)
    ctx.sync()
    ctx.record(e0)
    for _ in range(MAPS):
        m.compute_device(d_l, d_r, W, H, W, d_d)
    ctx.record(e1)
    ms = ctx.elapsed_ms(e0, e1) / MAPS
    ctx.set_profiling(True)
    ctx.sgbm_profile()                                                  # drop earlier sums
    for _ in range(MAPS):
        m.compute_device(d_l, d_r, W, H, W, d_d)
    ctx.sync()
    prof = ctx.sgbm_profile()
    ctx.set_profiling(False)
    return ms, prof


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "sgbm_wide_c2.json")
    res = {"config": "3264x2448 depth2 parameters, synth.stereo_pair(W, H, D), one map in flight, device events; "
                     f"{WARMUP} warm-up and {MAPS} timed maps per leg, then {MAPS} profiled maps",
           "volume_bytes": {str(D): volume_bytes(D) for D in (256, 512)},
           "volume_bytes_ratio_512_over_256": volume_bytes(512) / volume_bytes(256), "legs": {}}
    ctx = None
    for D in (256, 512):
        L, R, _ = r3d.synth.stereo_pair(W, H, D)
        for name, mode in (("3way", r3d.STEREO_SGBM_MODE_SGBM_3WAY), ("hh", r3d.STEREO_SGBM_MODE_HH)):
            m = r3d.StereoSGBM_create(numDisparities=D, mode=mode, **KW)
            ctx = m.context
            bufs = (ctx.to_device(L), ctx.to_device(R), ctx.alloc(W * H * 2))
            ms, prof = measure(m, ctx, bufs)
            for p in bufs:
                ctx.free(p)
            res["legs"][f"{name}_D{D}"] = {"ms_per_map": ms, "kernel_ms": prof, "kernel_ms_sum": float(sum(prof.values()))}
            print(f"{name} D={D}: {ms:.3f} ms per map", flush=True)
            if D == 512 and name == "3way":
                got = m.compute(L, R)
                t = time.time()
                want = so.compute(L, R, so.make_params(numDisparities=D, **KW), nthreads=8)
                res["3way_D512_bit_exact_vs_oracle"] = bool(np.array_equal(got, want))
                res["3way_D512_pixels_differing"] = int((got != want).sum())
                res["3way_D512_valid_fraction_right_of_D"] = float((got[:, D:] >= 0).mean())
                res["oracle_host_s"] = time.time() - t
    ratios = {}
    for name, kernels in VOLUME_KERNELS.items():
        a, b = res["legs"][f"{name}_D256"], res["legs"][f"{name}_D512"]
        ratios[name] = {k: b["kernel_ms"][k] / a["kernel_ms"][k] for k in kernels if a["kernel_ms"].get(k) and k in b["kernel_ms"]}
        ratios[name]["map"] = b["ms_per_map"] / a["ms_per_map"]
    res["ratio_512_over_256"] = ratios
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
    return 0 if res.get("3way_D512_bit_exact_vs_oracle") else 1


if __name__ == "__main__":
    sys.exit(main())
