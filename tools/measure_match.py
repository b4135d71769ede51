"""Call times of the descriptor matcher on the device (DESIGN.md section 5 has one set of them): the host clock around
mskf_fe_match_batch, which ends in the wait for the batch (staging copy in, k_fe_match, copy out, the host's unpacking), for
437 x 437 descriptors with 1, 32 and 256 jobs that share the query and 1700 x 1700 with 1 job, cross-check off and on, ratio 0.8:
median, 10th and 90th percentile, minimum and maximum of 100 calls after 10 warm-up calls, the device otherwise idle.  The train
descriptors are query descriptors with 0 .. 12 bits flipped; the first job of every shape is compared with the numpy restatement.

    python tools/measure_match.py [out.json]
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
from msckf_stereo_c_amd.ctypes_types import MATCH, FeMatchArgs      # noqa: E402
import match_cases as MC                                    # noqa: E402
import match_reference as MR                                # noqa: E402

WARMUP, CALLS = 10, 100
out = {}
ctx = capi.Context(0)
L = ctx.L
L.mskf_fe_match_batch.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
for n, jobs in ((437, 1), (437, 32), (437, 256), (1700, 1)):
    rng = np.random.default_rng([n, jobs])
    q = MC.rand_desc(rng, n)
    trains = [MC.near_set(rng, q, n) for _ in range(jobs)]
    res = np.zeros((jobs, n), MATCH)
    for cross in (0, 1):
        args = (FeMatchArgs * jobs)(*[FeMatchArgs(n, n, q.ctypes.data, None, t.ctypes.data, None, 256, 0.8, cross, res[k].ctypes.data, -1) for k, t in enumerate(trains)])
        us = []
        for it in range(WARMUP + CALLS):
            t0 = time.perf_counter()
            rc = L.mskf_fe_match_batch(ctx.h, jobs, args)
            t1 = time.perf_counter()
            assert rc == 0, L.mskf_last_error()
            if it >= WARMUP:
                us.append((t1 - t0) * 1e6)
        want, want_n = MR.match(q, trains[0], ratio=0.8, cross_check=bool(cross))
        assert np.array_equal(res[0], want) and args[0].n_matches == want_n
        us = np.array(us)
        key = "%dx%d_jobs%d_cross%d" % (n, n, jobs, cross)
        out[key] = dict(us_median=round(float(np.median(us)), 1), us_p10=round(float(np.percentile(us, 10)), 1), us_p90=round(float(np.percentile(us, 90)), 1),
                        us_min=round(float(us.min()), 1), us_max=round(float(us.max()), 1), pairs=int(n) * n * jobs * (2 if cross else 1), n_matches_job0=int(want_n))
        print("mskf_fe_match_batch %s: median %.1f us (p10 %.1f, p90 %.1f, min %.1f, max %.1f), %d matches in job 0" % (
            key, out[key]["us_median"], out[key]["us_p10"], out[key]["us_p90"], out[key]["us_min"], out[key]["us_max"], want_n), flush=True)
ctx.close()
if len(sys.argv) > 1:
    json.dump(out, open(sys.argv[1], "w"), indent=1)
