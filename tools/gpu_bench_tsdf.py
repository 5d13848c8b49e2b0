"""Time of the TSDF volume (r3d_tsdf_integrate_f32_dev, r3d_tsdf_extract_point_cloud_dev) on a 16-frame sequence at 640x480.

    python tools/gpu_bench_tsdf.py [--repeats 10] [--out profiles/tsdf.json] [--mesh-out profiles/tsdf_mesh.json] [--lib other/libr3d_hip.so]

The frames are the synthetic height-field scene of tests/rgbd_scene.py along a smooth pose path (1.5 / -2 / 1 degrees and
6 / -3 / 4 cm from the first to the last frame), colour = the intensity plane x 255 in three channels, planes resident on the
device.  The volume has Open3D's documented example values, voxel_length = 4 / 512 and sdf_trunc = 0.04, RGB8.  One run resets
the volume and integrates the 16 frames; r3d_tsdf_stats carries the library's two event intervals of the last frame, touch_ms
(touch pass, counter read, slot assignment) and integrate_ms (the voxel update).  Per frame: medians over `repeats` runs after
two warm-up runs (the first of which also grows the pool), with every run listed.

bytes_touched_state is the figure of merit the design names: units touched x 4096 voxels x bytes per voxel (4 tsdf + 4 weight +
24 colour), read and written, and share_of_peak is that over integrate_ms against 8 TB/s.  It is an upper bound of what the
kernel moves: a column none of whose 16 voxels updates (outside the image, on a hole, far behind the surface) loads and stores
nothing.  The numpy restatement's host time for one frame stands beside it, the restatement's case A once more (the largest
normal difference of the GPU tests), and the two timed lines of the reference's own log as context: unknown hardware, no target.

The mesh leg (r3d_mesh_from_volume_dev on the same volume, its own file) times two calls with events on the context stream: the
counting call (both capacities 0: cube bytes, counts, unit offsets and the 16-byte read of the totals) and the whole call into
device arrays; emit_ms is their difference (vertices with their ids, then triangles).  bytes_minimum is what the passes cannot
avoid, the state once (units x 4096 x 8 B, or 32 B with colour) and the rows written; share_of_peak is that over the whole call
against 8 TB/s.  The cloud extraction's time on the same volume stands beside it."""
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
W, H, FRAMES = 640, 480, 16
VOXEL_LENGTH, SDF_TRUNC = 4.0 / 512, 0.04
BYTES_PER_VOXEL = 4 + 4 + 24
PEAK_BYTES_PER_S = 8e12


def _sha(path):
    with open(path, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


def mesh_leg(r3d, ctx, volume, repeats, ev, cloud):
    """extract_triangle_mesh of the volume as the frames left it -> the report for profiles/tsdf_mesh.json"""
    nv, nt = volume.mesh_counts()
    units = len(volume)
    d_out = [ctx.alloc(max(nv, 1) * 24), ctx.alloc(max(nv, 1) * 24), ctx.alloc(max(nt, 1) * 12)]
    count_runs, whole_runs = [], []
    for i in range(repeats + 2):
        ctx.record(ev[0])
        counts = volume.mesh_counts()
        ctx.record(ev[1])
        count_ms = ctx.elapsed_ms(ev[0], ev[1])
        ctx.record(ev[0])
        got = volume.extract_mesh_device(d_out[0], d_out[1], d_out[2], nv, nt)
        ctx.record(ev[1])
        assert counts == got == (nv, nt)
        if i >= 2:
            count_runs.append(count_ms)
            whole_runs.append(ctx.elapsed_ms(ev[0], ev[1]))
    for ptr in d_out:
        ctx.free(ptr)
    count_ms, whole_ms = statistics.median(count_runs), statistics.median(whole_runs)
    moved = units * 4096 * BYTES_PER_VOXEL + nv * 48 + nt * 12
    return dict(config=f"the volume of profiles/tsdf.json after its {FRAMES} frames ({units} units, RGB8); medians of {repeats} runs after two warm-up "
                       "runs; events on the context stream around r3d_mesh_from_volume_dev",
                vertices=nv, triangles=nt, units=units, count_ms=count_ms, whole_ms=whole_ms, emit_ms=whole_ms - count_ms,
                count_ms_runs=[round(x, 4) for x in count_runs], whole_ms_runs=[round(x, 4) for x in whole_runs],
                bytes_minimum=moved, share_of_peak=moved / (whole_ms * 1e-3) / PEAK_BYTES_PER_S,
                cloud_extract_ms=cloud["extract_ms"], cloud_points=cloud["points"],
                note="count_ms: the call with both capacities 0 (cube bytes, counts, offsets, the read of the totals); whole_ms: the call into device "
                     "arrays, which repeats the counting; emit_ms: their difference.  bytes_minimum: the state once (units x 4096 x 32 B) plus the "
                     "vertex, colour and triangle rows written; the passes also write and read the cube bytes (1 B per voxel) and the vertex ids "
                     "(12 B per voxel)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tsdf.json"))
    ap.add_argument("--mesh-out", default=os.path.join(ROOT, "profiles", "tsdf_mesh.json"))
    ap.add_argument("--lib", default=None, help="another build of libr3d_hip.so to time instead of lib/libr3d_hip.so")
    a = ap.parse_args()
    r3d = importlib.import_module("3d_reconstruction_project_amd")
    if a.lib:
        r3d._lib.use_library(a.lib)
    ref = importlib.import_module("tests.tsdf_ref")
    scene = importlib.import_module("tests.rgbd_scene")
    ctx = r3d.default_context()
    cam = scene.camera(W, H)
    poses = [scene.pose(1.5 * s, -2.0 * s, 1.0 * s, (0.06 * s, -0.03 * s, 0.04 * s)) for s in (k / (FRAMES - 1) for k in range(FRAMES))]
    frames = []
    for pose in poses:
        inten, depth = scene.render(W, H, pose, scene.HOLES)
        frames.append((depth, np.ascontiguousarray(np.repeat((inten * 255).astype(np.uint8)[..., None], 3, axis=2))))
    dev = [(ctx.to_device(d), ctx.to_device(c)) for d, c in frames]
    extrinsics = [np.linalg.inv(p) for p in poses]

    runs = []      # [run][frame] = (touch_ms, integrate_ms, touched, units)
    volume = r3d.ScalableTSDFVolume(VOXEL_LENGTH, SDF_TRUNC, r3d.TSDFVolumeColorType.RGB8)
    wall = []
    for i in range(a.repeats + 2):
        volume.reset()
        ctx.sync()
        rows = []
        t0 = time.perf_counter()
        for (d_depth, d_color), E in zip(dev, extrinsics):
            volume.integrate_device(d_depth, d_color, W, H, cam, E)
            st = volume.stats()                                   # waits for the frame
            rows.append((st["touch_ms"], st["integrate_ms"], st["touched"], st["units"]))
        if i >= 2:
            runs.append(rows)
            wall.append((time.perf_counter() - t0) * 1e3)
    per_frame = []
    for k in range(FRAMES):
        touch = statistics.median(r[k][0] for r in runs)
        integ = statistics.median(r[k][1] for r in runs)
        touched, units = runs[0][k][2], runs[0][k][3]
        assert all(r[k][2] == touched and r[k][3] == units for r in runs)
        moved = touched * 4096 * BYTES_PER_VOXEL * 2
        per_frame.append(dict(frame=k, touch_ms=touch, integrate_ms=integ, units_touched=touched, units=units,
                              voxels_walked_per_s=touched * 4096 / (integ * 1e-3), bytes_touched_state=moved,
                              share_of_peak=moved / (integ * 1e-3) / PEAK_BYTES_PER_S,
                              integrate_ms_runs=[round(r[k][1], 4) for r in runs], touch_ms_runs=[round(r[k][0], 4) for r in runs]))
    n = volume.point_count()
    d_out = [ctx.alloc(max(n, 1) * 24) for _ in range(3)]
    ev = [ctx.event(), ctx.event()]
    extract_runs = []
    for i in range(a.repeats + 2):
        ctx.record(ev[0])
        got = volume.extract_device(d_out[0], d_out[1], d_out[2], n)
        ctx.record(ev[1])
        assert got == n
        if i >= 2:
            extract_runs.append(ctx.elapsed_ms(ev[0], ev[1]))
    st = volume.stats()
    report = dict(config=f"{FRAMES} frames {W}x{H} of the synthetic height-field scene along a smooth pose path, device planes; voxel_length 4/512, "
                         f"sdf_trunc 0.04, RGB8, stride 4; medians of {a.repeats} runs (reset + {FRAMES} frames) after two warm-up runs; touch_ms / "
                         "integrate_ms are the library's event intervals",
                  library_sha256=_sha(r3d._lib.LIB_PATH), tsdf_hip_sha256=_sha(os.path.join(ROOT, "3d_reconstruction_project_amd", "csrc", "tsdf.hip")),
                  per_frame=per_frame,
                  sequence=dict(touch_ms=sum(f["touch_ms"] for f in per_frame), integrate_ms=sum(f["integrate_ms"] for f in per_frame),
                                wall_ms=statistics.median(wall), wall_ms_runs=[round(w, 3) for w in wall], units=st["units"],
                                pool_capacity=st["capacity"], growths=st["growths"],
                                note="wall_ms: host time of one run, 16 x (integrate + r3d_tsdf_stats, which waits for the frame)"),
                  extract=dict(extract_ms=statistics.median(extract_runs), points=n, extract_ms_runs=[round(x, 4) for x in extract_runs],
                               note="count + unit offsets + emit into device arrays (r3d_tsdf_extract_point_cloud_dev), events on the context stream"))
    mesh_report = mesh_leg(r3d, ctx, volume, a.repeats, ev, report["extract"])
    mesh_report["library_sha256"], mesh_report["tsdf_hip_sha256"] = report["library_sha256"], report["tsdf_hip_sha256"]
    with open(a.mesh_out, "w") as f:
        json.dump(mesh_report, f, indent=1)
    print(json.dumps(mesh_report))
    t0 = time.perf_counter()
    host = ref.Volume(VOXEL_LENGTH, SDF_TRUNC, True, 4)
    host.integrate(frames[0][0], frames[0][1], cam, extrinsics[0])
    report["restatement"] = dict(host_ms_one_frame=(time.perf_counter() - t0) * 1e3, units=len(host.units),
                                 note="tests/tsdf_ref.py, vectorised numpy on the host of the run, frame 0 into an empty volume")
    # case A of tests/test_tsdf_gpu.py once more, for the record of its largest normal difference
    gpu_tests = importlib.import_module("tests.test_tsdf_gpu")
    _, cloud = gpu_tests._case_a()
    with r3d.ScalableTSDFVolume(0.01, 0.04, r3d.TSDFVolumeColorType.RGB8, initial_units=8) as small:
        for k, pose in enumerate(gpu_tests.POSES_A):
            depth, color = gpu_tests._frame(64, 48, k)
            small.integrate_f32(depth, color, scene.camera(64, 48), np.linalg.inv(pose))
        p, nrm, col = small.extract_arrays()
    report["case_a"] = dict(points=len(p), points_equal=bool(p.tobytes() == cloud[0].tobytes()), colours_equal=bool(col.tobytes() == cloud[2].tobytes()),
                            normals_max_abs_difference=float(np.abs(nrm - cloud[1]).max()), normals_bound=2.0 ** -50)
    report["reference_log"] = dict(runs=[dict(seconds=8.9, frames=76, ms_per_frame=8.9 / 76 * 1e3), dict(seconds=10.6, frames=87, ms_per_frame=10.6 / 87 * 1e3)],
                                   note="BASELINE.md section 1: ScalableTSDFVolume integration in the reference's own log, unknown hardware; context, not a target")
    for pair in dev:
        for ptr in pair:
            ctx.free(ptr)
    for ptr in d_out:
        ctx.free(ptr)
    volume.close()
    with open(a.out, "w") as f:
        json.dump(report, f, indent=1)
    print(json.dumps({k: v for k, v in report.items() if k != "per_frame"}))
    print("frame touch_ms integrate_ms touched share")
    for fr in per_frame:
        print(fr["frame"], round(fr["touch_ms"], 4), round(fr["integrate_ms"], 4), fr["units_touched"], round(fr["share_of_peak"], 4))


if __name__ == "__main__":
    main()
