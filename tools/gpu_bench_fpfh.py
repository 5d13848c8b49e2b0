"""Per-stage device time of the FPFH features and the feature matching at three sizes.

    python tools/gpu_bench_fpfh.py [--repeats 5] [--out profiles/fpfh.json] [--skip-1m]

Sizes: the recorded frame tests/golden/output/pcd_00008.ply (11 258 points, radius 0.1, as the reference's script calls it);
200 k and 1 M points of synth.cloud_pair's surface (3.5 mm spacing; the 1 M cloud is config C3's) with radius 0.05 = 5 x the
10 mm voxel, kNN-20 normals.  max_nn = 100 everywhere.

Per size, medians over `repeats` calls of r3d_debug_fpfh_stages after one warm-up (hipEvents around the kernels, one process):
    search_ms   k_knn_graph at the same (n, k, radius) on the same grid: the search both feature stages share, their floor
    spfh_ms     k_spfh (search + lists + histogram, with the gather of the normals);  spfh_over_search = the ratio
    fpfh_ms     k_fpfh
    total_ms    one r3d_compute_fpfh_dev call end to end (grid build included), events around the call
    match_ms    r3d_match_features_dev: frame 8 against frame 9; 100 000 x 100 000 rows of the 200 k cloud's features (its two
                halves); not run at 1 M (10^12 pairs)
and once, on the recorded frame, the wall time of the numpy restatement (tests/fpfh_ref.py) on the host.
The reference's only timing, 0.56-1.28 s per frame for a preprocessing step that includes FPFH, was taken on
unknown hardware and covers more than FPFH: it is quoted in the output as context, not as a pass mark."""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MAX_NN = 100


def measure(r3d, ctx, p, nm, radius, repeats, match):
    co = r3d.cloud_ops
    n = len(p)
    d_p, d_n, d_f = ctx.to_device(p), ctx.to_device(nm), ctx.alloc(n * 33 * 8)
    e0, e1 = ctx.event(), ctx.event()
    out = dict(n=n, radius=radius, max_nn=MAX_NN)
    try:
        co.debug_fpfh_stages(d_p, d_n, n, radius, d_f, MAX_NN, ctx=ctx)                    # warm-up
        runs = [co.debug_fpfh_stages(d_p, d_n, n, radius, d_f, MAX_NN, ctx=ctx) for _ in range(repeats)]
        for key in ("search_ms", "spfh_ms", "fpfh_ms"):
            out[key] = statistics.median(r[key] for r in runs)
            out[key + "_runs"] = [r[key] for r in runs]
        out["spfh_over_search"] = out["spfh_ms"] / out["search_ms"]
        out["fpfh_over_search"] = out["fpfh_ms"] / out["search_ms"]
        total = []
        for _ in range(repeats):
            ctx.record(e0)
            co.compute_fpfh_feature_device(d_p, d_n, n, radius, d_f, MAX_NN, ctx=ctx)
            ctx.record(e1)
            total.append(ctx.elapsed_ms(e0, e1))
        out["total_ms"] = statistics.median(total)
        if match is not None:
            (d_s, ns), (d_t, nt) = match(d_f)
            d_nn, d_d2 = ctx.alloc(ns * 4), ctx.alloc(ns * 8)
            ms = []
            for _ in range(repeats + 1):
                ctx.record(e0)
                co.match_features_device(d_s, ns, d_t, nt, d_nn, d_d2, ctx=ctx)
                ctx.record(e1)
                ms.append(ctx.elapsed_ms(e0, e1))
            out.update(match_ns=ns, match_nt=nt, match_ms=statistics.median(ms[1:]), match_ms_runs=ms[1:])
            ctx.free(d_nn)
            ctx.free(d_d2)
    finally:
        for b in (d_p, d_n, d_f):
            ctx.free(b)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fpfh.json"))
    ap.add_argument("--skip-1m", action="store_true")
    a = ap.parse_args()
    r3d = importlib.import_module("3d_reconstruction_project_amd")
    fr = importlib.import_module("tests.fpfh_ref")
    co, ctx = r3d.cloud_ops, r3d.default_context(0)
    report = dict(config=f"max_nn {MAX_NN}; golden: radius 0.1; synthetic: radius 0.05, kNN-20 normals; medians of {a.repeats}",
                  reference_context="0.56-1.28 s per frame for preprocessing that includes FPFH (r = 0.1, k <= 100), 9.6-15.6 s per "
                                    "pair for feature-matching registration; unknown hardware (BASELINE.md): context, not a pass mark")
    frames = [r3d.io_formats.read_ply(os.path.join(ROOT, "tests", "golden", "output", f"pcd_{f:05d}.ply")) for f in (8, 9)]
    p8, n8 = frames[0]["points"], frames[0]["normals"]

    def golden_match(d_f8):
        f9 = np.ascontiguousarray(co.compute_fpfh_feature(frames[1]["points"], frames[1]["normals"], 0.1, MAX_NN, ctx=ctx).T)
        golden_match.d = ctx.to_device(f9)
        return (d_f8, len(p8)), (golden_match.d, len(f9))

    report["golden_frame"] = measure(r3d, ctx, p8, n8, 0.1, a.repeats, golden_match)
    ctx.free(golden_match.d)
    t0 = time.perf_counter()
    idx, d2 = fr.neighbors(p8, 0.1, MAX_NN)
    t1 = time.perf_counter()
    spfh, _ = fr.spfh_vectorised(p8, n8, idx)
    t2 = time.perf_counter()
    fr.fpfh_stage_vectorised(spfh, idx, d2)
    t3 = time.perf_counter()
    report["golden_frame"]["host_restatement_s"] = dict(search=t1 - t0, spfh=t2 - t1, fpfh=t3 - t2, total=t3 - t0)
    for key, n in (("synthetic_200k", 200_000), ("c3_1m", 1_000_000)):
        if n == 1_000_000 and a.skip_1m:
            continue
        p = r3d.synth.cloud_pair(n, scale=(n / 1e6) ** 0.5)[1].astype(np.float64)
        nm = co.estimate_normals(p, None, 20, ctx=ctx)
        half = lambda d_f: ((d_f, 100_000), (d_f + 100_000 * 33 * 8, 100_000))       # noqa: E731
        report[key] = measure(r3d, ctx, p, nm, 0.05, a.repeats, half if n == 200_000 else None)
        print(key, json.dumps(report[key]), flush=True)
    with open(a.out, "w") as f:
        json.dump(report, f, indent=1)
    print(json.dumps(report))


if __name__ == "__main__":
    main()
