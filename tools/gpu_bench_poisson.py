"""Time of the Poisson reconstruction (r3d_poisson_reconstruct_dev) and of its stages.

    python tools/gpu_bench_poisson.py [--repeats 10] [--out profiles/poisson.json]

Inputs: the fixture frame tests/golden/output/pcd_00008.ply (11 258 points with the reference's normals and colours) at depth 6,
and a 1 000 000-point sphere of radius 0.7 (Fibonacci lattice, radial noise 0.001, outward normals, colours) at depths 6, 7 and 8.
Arrays are resident on the device.  call_ms is the interval between two events on the context stream around one call, which returns
once the mesh is complete: the median of `repeats` calls after two warm-up calls, every run listed.  stage_ms comes from the
library's own events on the same stream (r3d_set_profiling), one per stage boundary, medians over the same number of calls:
  ordering    bounds and their read, the cell sort, first point per cell, fractions
  splats      gather, density pass, gather
  solve       divergence, coarse diagonals, the V-cycles
  extraction  cube bytes, counts, two scans, the read of the counts, vertices and triangles
sweep_ms is (solve with pre = post = 12 - solve with pre = post = 2) / (20 cycles): one Jacobi sweep of EVERY level, an upper bound
of the finest level's; sweep_bytes = 4 fields of G^3 float64 (three read, one written); share_of_peak against 8 TB/s.
numpy_ms is tests/poisson_ref.py on the host of the run for the same work, where it is expected within a minute."""
import argparse
import hashlib
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK_BYTES_PER_S = 8e12
STAGES = ("ordering", "splats", "solve", "extraction")


def _sha(path):
    with open(path, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


def bench(r3d, ctx, name, pts, nrm, col, depth, repeats, numpy_too):
    po = r3d.poisson
    ref = importlib.import_module("tests.poisson_ref")
    n, G = len(pts), (1 << depth) + 1
    d_in = [ctx.to_device(a) for a in (pts, nrm, col)]
    prm = po.poisson_params(depth=depth)
    nv, nt = po.reconstruct_device(*d_in, n, prm, 0, 0, None, None, None, None, ctx=ctx)
    d_out = [ctx.alloc(max(nv, 1) * 24), ctx.alloc(max(nv, 1) * 8), ctx.alloc(max(nv, 1) * 24), ctx.alloc(max(nt, 1) * 12)]
    ev = [ctx.event(), ctx.event()]

    def call(p):
        if p is not prm:            # other sweep counts move the surface by a few vertices: the counts alone, the solve is the same
            return po.reconstruct_device(*d_in, n, p, 0, 0, None, None, None, None, ctx=ctx)
        return po.reconstruct_device(*d_in, n, p, nv, nt, *d_out, ctx=ctx)

    def timed(p):
        runs = []
        for i in range(repeats + 2):
            ctx.record(ev[0])
            assert call(p) == (nv, nt)
            ctx.record(ev[1])
            if i >= 2:
                runs.append(ctx.elapsed_ms(ev[0], ev[1]))
        return statistics.median(runs), [round(x, 4) for x in runs]

    def stages(p):
        ctx.set_profiling(True)
        ctx.sgbm_profile()                      # drop what earlier calls left
        rows = []
        for _ in range(repeats):
            call(p)
            got = ctx.sgbm_profile()
            rows.append([got.get("poisson_" + s, float("nan")) for s in STAGES])
        ctx.set_profiling(False)
        return {s: statistics.median(r[k] for r in rows) for k, s in enumerate(STAGES)}

    out = dict(input=name, points=n, depth=depth, nodes_per_axis=G, vertices=nv, triangles=nt)
    out["call_ms"], out["call_ms_runs"] = timed(prm)
    out["stage_ms"] = stages(prm)
    long = po.poisson_params(depth=depth, pre=12, post=12)
    solve_long = stages(long)["solve"]
    out["solve_ms_pre_post_12"] = solve_long
    out["sweep_ms"] = (solve_long - out["stage_ms"]["solve"]) / (20 * prm.cycles)
    out["sweep_bytes"] = 4 * G ** 3 * 8
    out["sweep_share_of_peak"] = out["sweep_bytes"] / (out["sweep_ms"] * 1e-3) / PEAK_BYTES_PER_S if out["sweep_ms"] > 0 else None
    if numpy_too:
        got = [np.empty((nv, 3)), np.empty(nv), np.empty((nv, 3)), np.empty((nt, 3), np.int32)]
        call(prm)
        for a, d in zip(got, d_out):
            if a.size:
                ctx.d2h(a, d)
        t0 = time.perf_counter()
        want = ref.reconstruct(pts, nrm, col, ref.params(depth=depth), r3d.tsdf.mc_table())
        out["numpy_ms"] = (time.perf_counter() - t0) * 1e3
        out["equals_restatement"] = bool(all(a.tobytes() == w.tobytes() for a, w in zip(got, want)))
    for d in d_in + d_out:
        ctx.free(d)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "poisson.json"))
    a = ap.parse_args()
    r3d = importlib.import_module("3d_reconstruction_project_amd")
    ref = importlib.import_module("tests.poisson_ref")
    ctx = r3d.default_context()
    ply = r3d.io_formats.read_ply(os.path.join(ROOT, "tests", "golden", "output", "pcd_00008.ply"))
    frame = tuple(np.ascontiguousarray(ply[k], dtype=np.float64) for k in ("points", "normals", "colors_f"))
    sphere = ref.sphere_cloud(1_000_000, 0.7, noise=0.001, seed=1, lattice=True)
    cases = [bench(r3d, ctx, "tests/golden/output/pcd_00008.ply", *frame, 6, a.repeats, True)]
    for depth in (6, 7, 8):
        # the restatement beside the device where it is expected within a minute: its time grows 8x per depth
        within = depth == 6 or cases[-1].get("numpy_ms", 1e9) * 8 < 60e3
        cases.append(bench(r3d, ctx, "sphere, 1 000 000 points", *sphere, depth, a.repeats, within))
    report = dict(config=f"medians of {a.repeats} calls after two warm-up calls; events on the context stream around r3d_poisson_reconstruct_dev, arrays "
                         "resident; stage_ms from the library's events at the stage boundaries; defaults: 10 cycles, pre = post = 2, 40 coarsest sweeps",
                  library_sha256=_sha(r3d._lib.LIB_PATH), poisson_hip_sha256=_sha(os.path.join(ROOT, "3d_reconstruction_project_amd", "csrc", "poisson.hip")),
                  cases=cases,
                  note="sweep_ms: (solve with pre = post = 12 - solve with pre = post = 2) / 200, one sweep of every level; sweep_bytes: 4 G^3 float64; "
                       "share against 8 TB/s")
    with open(a.out, "w") as f:
        json.dump(report, f, indent=1)
    print(json.dumps(report))


if __name__ == "__main__":
    main()
