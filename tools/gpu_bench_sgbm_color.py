"""SGBM at 3264x2448, D = 128, blockSize 5 (the reference's depth2 parameters) on a grey pair and on a 3-channel pair, in ONE
process: MODE_SGBM_3WAY and MODE_HH, one map in flight: ms per map (device events, after warm-up, 10 timed maps) and per-kernel
ms (r3d_set_profiling / sgbm_profile over 10 further maps).  A colour map runs the cost kernel once per channel, the second and
third launch adding to the stored volume; the condition checked here is that it costs less than three grey maps of its mode
(three grey runs being the trivial way to three block costs).  Also compared on the GPU: equal channels with three times the
penalties give the grey map bit for bit as long as no path sum saturates (3WAY; recorded, not a condition).
Usage (GPU box): python tools/gpu_bench_sgbm_color.py [out.json]   (default: profiles/sgbm_color_c2.json)"""
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
r3d = importlib.import_module("3d_reconstruction_project_amd")

W, H, D = 3264, 2448, 128
KW = dict(minDisparity=0, blockSize=5, P1=600, P2=2400, disp12MaxDiff=1, uniquenessRatio=15, speckleWindowSize=0,
          speckleRange=2, preFilterCap=63)           # Calib_depth/depth2.py:146-158
WARMUP, MAPS = 3, 10


def colour(g, rng):
    """The grey image scaled by 0.8 / 1.0 / 0.9 per channel plus 0..11 of per-channel noise (the recipe of the colour tests)."""
    out = np.empty(g.shape + (3,), np.uint8)
    for c, s in enumerate((0.8, 1.0, 0.9)):
        out[:, :, c] = np.clip(g * np.float32(s) + rng.integers(0, 12, g.shape), 0, 255).astype(np.uint8)
    return out


def measure(m, ctx, bufs, cn):
    d_l, d_r, d_d = bufs

    def run():
        m.compute_device(d_l, d_r, W, H, W * cn, d_d, channels=cn)
    e0, e1 = ctx.event(), ctx.event()
    for _ in range(WARMUP):
        run()
    ctx.sync()
    ctx.record(e0)
    for _ in range(MAPS):
        run()
    ctx.record(e1)
    ms = ctx.elapsed_ms(e0, e1) / MAPS
    ctx.set_profiling(True)
    ctx.sgbm_profile()                                                  # drop earlier sums
    for _ in range(MAPS):
        run()
    ctx.sync()
    prof = ctx.sgbm_profile()
    ctx.set_profiling(False)
    return ms, prof


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "sgbm_color_c2.json")
    res = {"config": f"{W}x{H} D={D} depth2 parameters, synth.stereo_pair and its colour version, one map in flight, device "
                     f"events; {WARMUP} warm-up and {MAPS} timed maps per leg, then {MAPS} profiled maps",
           "volume_bytes": (W - D) * H * D * 2, "legs": {}}
    Lg, Rg, _ = r3d.synth.stereo_pair(W, H, D)
    rng = np.random.default_rng(1)
    pairs = {"grey": (Lg, Rg, 1), "colour": (colour(Lg, rng), colour(Rg, rng), 3)}
    maps = {}
    for name, mode in (("3way", r3d.STEREO_SGBM_MODE_SGBM_3WAY), ("hh", r3d.STEREO_SGBM_MODE_HH)):
        for kind, (L, R, cn) in pairs.items():
            m = r3d.StereoSGBM_create(numDisparities=D, mode=mode, **KW)
            ctx = m.context
            bufs = (ctx.to_device(L), ctx.to_device(R), ctx.alloc(W * H * 2))
            ms, prof = measure(m, ctx, bufs, cn)
            got = np.empty((H, W), np.int16)
            ctx.d2h(got, bufs[2])
            for p in bufs:
                ctx.free(p)
            maps[name, kind] = got
            res["legs"][f"{name}_{kind}"] = {"ms_per_map": ms, "kernel_ms": prof, "kernel_ms_sum": float(sum(prof.values())),
                                             "valid_fraction_right_of_D": float((got[:, D:] >= 0).mean())}
            print(f"{name} {kind}: {ms:.3f} ms per map, cost {prof.get('cost', float('nan')):.3f} ms", flush=True)
        g, c = res["legs"][f"{name}_grey"], res["legs"][f"{name}_colour"]
        res[f"{name}_colour_over_grey"] = c["ms_per_map"] / g["ms_per_map"]
        res[f"{name}_colour_cost_over_grey_cost"] = c["kernel_ms"]["cost"] / g["kernel_ms"]["cost"]
        res[f"{name}_colour_map_differs_from_grey_map_fraction"] = float((maps[name, "colour"] != maps[name, "grey"]).mean())
    # equal channels, three times the penalties: the grey map (3WAY)
    L3, R3 = (np.ascontiguousarray(np.repeat(a[:, :, None], 3, 2)) for a in (Lg, Rg))
    m3 = r3d.StereoSGBM_create(numDisparities=D, mode=r3d.STEREO_SGBM_MODE_SGBM_3WAY, **dict(KW, P1=3 * KW["P1"], P2=3 * KW["P2"]))
    res["3way_equal_channels_x3_penalties_equal_grey_map"] = bool(np.array_equal(m3.compute(L3, R3), maps["3way", "grey"]))
    res["colour_map_under_three_grey_maps"] = bool(all(res[f"{n}_colour_over_grey"] < 3.0 for n in ("3way", "hh")))
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
    return 0 if res["colour_map_under_three_grey_maps"] else 1


if __name__ == "__main__":
    sys.exit(main())
