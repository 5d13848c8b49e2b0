"""Times PointCloudAlignment.align_point_clouds (main.py:48) on the recorded fixture frames (config C4 sizes: ~280 k raw
points per frame, ~40 k after voxel 0.01) and on a growing model, as the scanning loop does.  Run on the GPU box.
--lib PATH times another build of the library (e.g. the parent commit's) instead of lib/libr3d_hip.so."""
import importlib, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
r3d = importlib.import_module("3d_reconstruction_project_amd")
if "--lib" in sys.argv:
    r3d._lib.use_library(sys.argv[sys.argv.index("--lib") + 1], allow_missing=True)
from oracle import cloud_oracle as co
G = os.path.join(os.path.dirname(__file__), "..", "tests", "golden")
intr = co.read_intrinsics(os.path.join(G, "camera_intrinsic.json"))
frames = [co.backproject(co.read_png16(os.path.join(G, f"output84/depth_{i:05d}.png")), intr)[0] for i in range(8, 16)]
pa = r3d.PointCloudAlignment(verbose=False)
pa.align_point_clouds(r3d.PointCloud(frames[1]), r3d.PointCloud(frames[0]))      # warm-up
out = {"raw_points_per_frame": int(np.mean([len(f) for f in frames]))}
ts = []
for i in range(1, 8):
    t0 = time.perf_counter()
    a = pa.align_point_clouds(r3d.PointCloud(frames[i]), r3d.PointCloud(frames[i - 1]))
    ts.append((time.perf_counter() - t0, pa.last_result["iterations"], pa.last_result["setup_ms"], pa.last_result["loop_ms"], len(a.points)))
out["pairwise"] = {"ms": round(1e3 * float(np.median([t[0] for t in ts])), 2), "iterations": [t[1] for t in ts],
                   "setup_ms": round(float(np.median([t[2] for t in ts])), 2), "loop_ms": round(float(np.median([t[3] for t in ts])), 2),
                   "points_after_voxel": ts[0][4]}
feed = [r3d.PointCloud(f) for f in frames]
for rep in range(3):      # the first pass grows the device arena to the size of the largest model (one-off allocations)
    log = []
    t0 = time.perf_counter()
    model = r3d.pipeline.fuse(feed, flavour="icp", log=log)
    out["fuse_8_frames_ms" if rep else "fuse_8_frames_first_pass_ms"] = round(1e3 * (time.perf_counter() - t0), 1)
out["model_points"] = len(model.points)
out["per_frame"] = {"setup_ms": [round(r["setup_ms"], 2) for r in log], "loop_ms": [round(r["loop_ms"], 2) for r in log],
                    "iterations": [r["iterations"] for r in log]}
out["sum_setup_ms"] = round(sum(r["setup_ms"] for r in log), 2)
out["sum_loop_ms"] = round(sum(r["loop_ms"] for r in log), 2)
# pieces outside the registration calls: first-frame upload and the final download
m = r3d.cloud_ops.ResidentModel()
t0 = time.perf_counter(); m.append(frames[0]); r3d.default_context().sync(); out["first_frame_append_ms"] = round(1e3 * (time.perf_counter() - t0), 2)
m.close()
t0 = time.perf_counter(); r3d.pipeline.fuse(feed, flavour="icp", resident=False); out["fuse_8_frames_host_model_ms"] = round(1e3 * (time.perf_counter() - t0), 1)
depths = [co.read_png16(os.path.join(G, f"output84/depth_{i:05d}.png")) for i in range(8, 16)]
cam = r3d.cloud_ops.depth_camera(intr)
r3d.pipeline.fuse_depth_frames(depths, cam)
ts = []
for rep in range(3):
    t0 = time.perf_counter(); md = r3d.pipeline.fuse_depth_frames(depths, cam); ts.append(time.perf_counter() - t0)
out["fuse_8_depth_images_ms"] = round(1e3 * min(ts), 1)
out["depth_loop_equals_cloud_loop"] = bool(np.array_equal(md.points, model.points))
print(json.dumps(out))
