"""Call times of the geometric verification on the device (DESIGN.md section 5 has one set of them): the host clock around
mskf_fe_verify_batch, which covers the host's triangulation and compaction, the staging copy in, k_fe_verify, the copy of the keys
out, the wait, and the host's inlier marking and refinement, for one shape given on the command line: pairs, hypotheses, jobs
(437 256 1, 437 256 256 and 1700 1024 1 are the shapes of DESIGN.md; run each as a process of its own under its own time limit).
Median, 10th and 90th percentile, minimum and maximum of 100 calls after 10 warm-up calls, the device otherwise idle.  Half of the
pairs are wrong, the noise is 0.5 px; the first job is compared with the Python restatement.

    timeout 120 python tools/measure_verify.py 437 256 1 [out.json]
"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from msckf_stereo_c_amd import capi                         # noqa: E402
from msckf_stereo_c_amd.ctypes_types import FeVerifyArgs    # noqa: E402
import verify_cases as VC                                   # noqa: E402
import verify_reference as VR                               # noqa: E402

WARMUP, CALLS = 10, 100
n, K, jobs = (int(v) for v in sys.argv[1:4])
ctx = capi.Context(0)
L = ctx.L
L.mskf_fe_verify_batch.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
scenes = [VC.scene(1000 + k, n, wrong=0.5, noise_px=0.5) for k in range(jobs)]
inl = np.zeros((jobs, n), np.uint8)
args = (FeVerifyArgs * jobs)()
for k, (q, t, _, _, _) in enumerate(scenes):
    a = args[k]
    a.n, a.n_hypotheses, a.query_obs, a.train_obs, a.usable = n, K, q.ctypes.data, t.ctypes.data, None
    a.T_cam1_cam0[:] = VC.T10.reshape(-1).tolist()
    a.seed, a.max_error, a.min_depth, a.max_depth, a.inlier = 7 + k, VC.MAX_ERROR, VC.MIN_DEPTH, VC.MAX_DEPTH, inl[k].ctypes.data
us = []
for it in range(WARMUP + CALLS):
    t0 = time.perf_counter()
    rc = L.mskf_fe_verify_batch(ctx.h, jobs, args)
    t1 = time.perf_counter()
    assert rc == 0, L.mskf_last_error()
    if it >= WARMUP:
        us.append((t1 - t0) * 1e6)
want = VR.verify(scenes[0][0], scenes[0][1], VC.T10, VC.MAX_ERROR, n_hypotheses=K, seed=7)
a = args[0]
assert (a.n_usable, a.n_inliers, a.best, a.status) == tuple(want[k] for k in ("n_usable", "n_inliers", "best", "status")), (a.n_usable, a.n_inliers, a.best, a.status)
assert np.array_equal(inl[0], want["inlier"]) and a.R[:] == want["R"].reshape(-1).tolist() and a.t[:] == want["t"].tolist() and a.rms == want["rms"]
us = np.array(us)
key = "%dx%d_jobs%d" % (n, K, jobs)
out = {key: dict(us_median=round(float(np.median(us)), 1), us_p10=round(float(np.percentile(us, 10)), 1), us_p90=round(float(np.percentile(us, 90)), 1),
                 us_min=round(float(us.min()), 1), us_max=round(float(us.max()), 1), evaluations=n * K * jobs, n_inliers_job0=int(a.n_inliers))}
print("mskf_fe_verify_batch %s: median %.1f us (p10 %.1f, p90 %.1f, min %.1f, max %.1f), %d inliers of %d usable in job 0" % (
    key, out[key]["us_median"], out[key]["us_p10"], out[key]["us_p90"], out[key]["us_min"], out[key]["us_max"], a.n_inliers, a.n_usable), flush=True)
ctx.close()
if len(sys.argv) > 4:
    json.dump(out, open(sys.argv[4], "w"), indent=1)
