"""bench.py's options, without a GPU: a plain run has no second window, --full has it; --steps is validated; --dump-outputs
writes float32 / float64 arrays of the timed path's last step (stream 0's trajectory cut at that step).  The checks run in a
child process: importing bench.py sets the HIP queue count of the process that imports it."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r'''
import os, sys, tempfile
import numpy as np
sys.path.insert(0, sys.argv[1])
import bench
from msckf_stereo_c_amd.ctypes_types import POINT2F, POSE

plain = bench.parse(["--gpus", "1", "--steps", "20", "--warmup", "5"])
assert not plain.full and plain.gram_steps == 0 and plain.dump_outputs is None
full = bench.parse(["--gpus", "1", "--steps", "20", "--warmup", "5", "--full"])
assert full.full and full.gram_steps == 12
for bad in (["--steps", "0"], ["--warmup", "-1"]):
    try:
        bench.parse(bad)
        raise AssertionError("accepted %s" % bad)
    except SystemExit as e:
        assert e.code == 2


class FakeRun:
    def mark_dump(self, g):
        n = 3 + g
        c = np.zeros(n, POINT2F)
        c["x"], c["y"] = np.arange(n), g
        return np.arange(n, dtype=np.uint64), np.ones(n, np.int32), c, c, np.full(28, float(g))

    def poses(self, s):
        p = np.zeros(200, POSE)
        p["t"] = (bench.T0_NS + np.arange(200) * bench.FRAME_DT_NS) * 1e-9
        return p


d = tempfile.mkdtemp()
bench.write_outputs(bench.collect_outputs(FakeRun(), plain, 4, 192, True), d)
got = {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}
assert all(a.dtype in (np.float32, np.float64) for a in got.values())
assert got["features_per_group"].tolist() == [3, 4, 5, 6] and got["feature_cam0_px"].shape == (18, 2)
assert got["imu_state"].shape == (4, 28) and got["imu_state"][3, 0] == 3.0
assert got["pose_stream0"].shape == (plain.prime + plain.warmup + plain.steps, 8)
print("ok")
'''


def test_bench_options_and_output_dump():
    p = subprocess.run([sys.executable, "-c", CHILD, ROOT], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.strip() == "ok", p.stdout + p.stderr
