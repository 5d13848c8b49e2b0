"""bench.py on the GPU: a plain run prints the headline alone, and --dump-outputs writes what the timed path computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, D = 3264, 2448, 128
C2_KW = dict(minDisparity=0, blockSize=5, P1=600, P2=2400, disp12MaxDiff=1, uniquenessRatio=15,
             speckleWindowSize=0, speckleRange=2, preFilterCap=63)


def test_plain_run_dumps_the_last_timed_map(r3d, tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["steps"] == 3 and out["warmup"] == 1 and out["dtype"] == "int16" and out["higher_is_better"] is True
    assert out["value"] > 0 and abs(out["value"] * out["ms_per_step"] / 1e3 - 1) < 1e-3       # both from the same timed region
    assert not {"roofline", "cpu_baseline", "pipelined", "secondary", "c5"} & set(out)           # those are --full's
    got = np.load(tmp_path / "disparity.npy")
    assert got.dtype == np.float32 and got.shape == (H, W)
    from oracle import sgbm_oracle as so
    L, R, _ = r3d.synth.stereo_pair(W, H, D, seed=20241008)                                     # rank 0's pair
    want = so.compute(L, R, so.make_params(numDisparities=D, **C2_KW), nthreads=8)
    np.testing.assert_array_equal(got, want.astype(np.float32))
