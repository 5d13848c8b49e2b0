"""Device time of the feature-matching RANSAC (r3d_ransac_correspondence_dev).

    python tools/gpu_bench_ransac.py [--repeats 5] [--out profiles/ransac.json]

Medians of `repeats` calls after one warm-up, hipEvents around the call (it returns when its loop has finished), one process:
    scripts_early_stop  recorded frames 8 -> 9 as the reference's scripts call it: voxel 0.05, normals Hybrid(0.1, 30), FPFH
                        Hybrid(0.25, 100), mutual filter, threshold 0.075, edge-length 0.9 and distance checkers, 4 M iterations,
                        confidence 0.999: ms per call, iterations, validated, batches
    scripts_all_4m      the same with confidence = 1: all 4 M hypotheses run.  This is what the reference's 9.6-15.6 s per pair
                        belong to (unknown hardware, and that call also builds the features): context, not a pass mark
    score_only          both checkers off, 10^5 hypotheses x 10^4 planted pairs, confidence 1: k_ransac_score alone, in effect.
                        Pair evaluations per second; float64 instructions per second counted from the source (per pair: 11 fma,
                        3 subtractions, 1 multiplication, 1 addition, 1 comparison = 17; 28 operations if an fma counts twice);
                        their ratio to k_match_features' measured rate (profiles/fpfh.json: 99 instructions per row pair, none
                        fused), the same broadcast-from-LDS shape
    host_restatement_s  tests/ransac_ref.py on the first case, wall time on the host, over at most the first 16 384 hypotheses (all of
                        the run when it stops before that)
    demonstration       frame 8 against its moved, thinned copy (tests/ransac_ref.frame_pair): the pose error of global_registration,
                        of multi_scale_icp started from it, and of multi_scale_icp started from identity"""
import argparse
import importlib
import json
import math
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BATCH = 65536                               # passed explicitly (it is also the library's default), so `batches` is exact
MATCH_RATE = 25e12                          # k_match_features, float64 instructions per second (profiles/fpfh.json, 10^5 x 10^5 rows)


def timed(co, ctx, src, tgt, corres, repeats, **kw):
    d_s, d_t, d_c = ctx.to_device(src), ctx.to_device(tgt), ctx.to_device(corres)
    e0, e1 = ctx.event(), ctx.event()
    ms, res = [], None
    try:
        for _ in range(repeats + 1):
            ctx.record(e0)
            res = co.registration_ransac_based_on_correspondence_device(d_s, len(src), d_t, len(tgt), d_c, len(corres), batch=BATCH, ctx=ctx, **kw)
            ctx.record(e1)
            ctx.sync()
            ms.append(ctx.elapsed_ms(e0, e1))
    finally:
        for d in (d_s, d_t, d_c):
            ctx.free(d)
    out = {k: res[k] for k in ("fitness", "inlier_rmse", "iterations", "validated", "best_hypothesis", "inliers", "setup_ms", "loop_ms")}
    out.update(pairs=len(corres), ms=statistics.median(ms[1:]), ms_runs=ms[1:], batches=math.ceil(res["iterations"] / BATCH))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ransac.json"))
    a = ap.parse_args()
    r3d = importlib.import_module("3d_reconstruction_project_amd")
    rr = importlib.import_module("tests.ransac_ref")
    co, ctx = r3d.cloud_ops, r3d.default_context(0)
    report = dict(config=f"medians of {a.repeats} after a warm-up; batch {BATCH}",
                  reference_context="9.6-15.6 s per pair, 86 pairs in 1 024 s, for feature-matching registration with 4 M iterations at "
                                    "confidence 0.999, features included; unknown hardware (BASELINE.md): context, not a pass mark")
    voxel = 0.05
    downs = []
    for f in (8, 9):
        pts = r3d.io_formats.read_ply(os.path.join(ROOT, "tests", "golden", "output", f"pcd_{f:05d}.ply"))["points"]
        down, _, _ = co.voxel_down_sample(pts, voxel, ctx=ctx)
        nrm = co.estimate_normals(down, voxel * 2, 30, ctx=ctx)
        downs.append((down, co.compute_fpfh_feature(down, nrm, voxel * 5, 100, ctx=ctx)))
    (sd, sf), (td, tf) = downs
    corres = co.correspondences_from_features(sf, tf, mutual_filter=True, ctx=ctx)
    kw = dict(max_correspondence_distance=voxel * 1.5, ransac_n=3, edge_length=0.9, checker_distance=voxel * 1.5, max_iteration=4_000_000, seed=0)
    report["scripts_early_stop"] = dict(source_points=len(sd), target_points=len(td), **timed(co, ctx, sd, td, corres, a.repeats, confidence=0.999, **kw))
    print("scripts_early_stop", json.dumps(report["scripts_early_stop"]), flush=True)
    report["scripts_all_4m"] = timed(co, ctx, sd, td, corres, a.repeats, confidence=1.0, **kw)
    print("scripts_all_4m", json.dumps(report["scripts_all_4m"]), flush=True)
    n_host = min(report["scripts_early_stop"]["iterations"], 16384)     # the restatement scores every validated hypothesis in numpy: bounded
    t0 = time.perf_counter()
    ref = rr.run(sd, td, corres, voxel * 1.5, 3, 0.9, voxel * 1.5, n_host, 0.999, 0, chunk=1024)
    report["host_restatement_s"] = dict(seconds=time.perf_counter() - t0, hypotheses=ref["iterations"], validated=ref["validated"],
                                        whole_run=n_host == report["scripts_early_stop"]["iterations"],
                                        same_best=ref["best_hypothesis"] == report["scripts_early_stop"]["best_hypothesis"])
    print("host_restatement_s", json.dumps(report["host_restatement_s"]), flush=True)

    src, tgt, pairs, _, _ = rr.planted_case(10_000, 4_000, seed=5)
    so = timed(co, ctx, src, tgt, pairs, a.repeats, max_correspondence_distance=0.02, ransac_n=3, edge_length=None, checker_distance=0,
               max_iteration=100_000, confidence=1.0, seed=0)
    evals = so["validated"] * so["pairs"]
    so.update(pair_evaluations=evals, pair_evaluations_per_s=evals / (so["loop_ms"] * 1e-3), f64_instructions_per_pair=17,
              f64_instructions_per_s=17 * evals / (so["loop_ms"] * 1e-3), f64_operations_per_s_fma_as_two=28 * evals / (so["loop_ms"] * 1e-3))
    so["ratio_to_match_features"] = so["f64_instructions_per_s"] / MATCH_RATE
    report["score_only"] = so
    print("score_only", json.dumps(so), flush=True)

    p, _, q, _, t_true = rr.frame_pair()
    pa = r3d.pointcloud_alignment
    t_g, res = pa.global_registration(p, q, 0.02, seed=0, max_iteration=100_000)
    t_gi, _ = pa.multi_scale_icp(res["source_down"], res["target_down"], 0.02, init=t_g, target_normals=res["target_normals"])
    t_id, _ = pa.multi_scale_icp(res["source_down"], res["target_down"], 0.02, init=None, target_normals=res["target_normals"])
    err = lambda t: float(np.abs(t - t_true).max())                 # noqa: E731
    report["demonstration"] = dict(pair="frame 8 vs its copy: 2 of 3 points, 1 rad about (1,2,3)/sqrt(14), shift (0.3,-0.2,0.5), 0.5 mm noise",
                                   voxel=0.02, source_points=len(res["source_down"]), target_points=len(res["target_down"]),
                                   ransac_inliers=res["inliers"], ransac_iterations=res["iterations"],
                                   max_abs_T_error_global_registration=err(t_g), max_abs_T_error_then_multi_scale_icp=err(t_gi),
                                   max_abs_T_error_multi_scale_icp_from_identity=err(t_id))
    with open(a.out, "w") as f:
        json.dump(report, f, indent=1)
    print(json.dumps(report))


if __name__ == "__main__":
    main()
