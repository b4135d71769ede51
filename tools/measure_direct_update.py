"""Times of the direct measurement update on the device (DESIGN.md section 5 has one set of them):

  * k_ekf_direct_update from the context's HIP-event timing (the MSKF_K_EKF_AUGMENT slot), three selector rows, d = 201 and 405,
    batches of 1 and 192 streams: median / min / max of 40 launches after 5 warm-up launches, and the rate at which the
    2 d^2 8 bytes per stream (one read and one write of P) move at the median;
  * the filter stage per frame (sum of the filter thread's phases, Runner.get_phases) of a 192-stream lockstep group over frames
    25..59 of the static lead-in of the zero-velocity tests' stream, with the zero-velocity update firing in every frame and with
    it off, the two Runners alternating in blocks of five frames.

    python tools/measure_direct_update.py [out.json]
"""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from msckf_stereo_c_amd import capi, runner as RN          # noqa: E402
from msckf_stereo_c_amd.ctypes_types import default_ekf_cfg, default_fe_cfg      # noqa: E402
from oracle import oracle_py                                # noqa: E402
import direct_update_reference as DR                        # noqa: E402

out = {}
oracle_py.build()
ctx = capi.Context(0)
L = ctx.L
L.mskf_ctx_set_timing.argtypes = [C.c_void_p, C.c_int]
L.mskf_ctx_get_timing.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
assert L.mskf_ctx_set_timing(ctx.h, 1) == 0
K = 14
ms, nl, nu = np.zeros(K), np.zeros(K, np.int64), np.zeros(K, np.int64)
calib = oracle_py.euroc_calib(64, 64)
for d in (201, 405):
    P = DR.make_P("spd", d)
    H, r, R = DR.make_measurement(P, 3, False, np.random.default_rng(1))
    for n in (1, 192):
        ss = [capi.Stream(ctx, calib, default_fe_cfg(), default_ekf_cfg(max_cam_state_size=(d - 21) // 6)) for _ in range(n)]
        for s in ss:
            s.ekf_set_cov(P)
        prs = [dict(H=H, r=r, R=R, pos_var=True)] * n
        for _ in range(5):
            ctx.ekf_update_direct_batch(ss, prs)
        L.mskf_ctx_get_timing(ctx.h, ms.ctypes.data, nl.ctypes.data, nu.ctypes.data, 1)
        reps = []
        for _ in range(40):
            res = ctx.ekf_update_direct_batch(ss, prs)
            L.mskf_ctx_get_timing(ctx.h, ms.ctypes.data, nl.ctypes.data, nu.ctypes.data, 1)
            assert nl[4] == 1 and res[0]["status"] == 1
            reps.append(float(ms[4]) * 1e3)
        reps = np.array(reps)
        byts = 2.0 * d * d * 8 * n
        med = float(np.median(reps))
        out["kernel_d%d_n%d" % (d, n)] = dict(us_median=round(med, 2), us_min=round(float(reps.min()), 2), us_max=round(float(reps.max()), 2),
                                              bytes=byts, GBps_at_median=round(byts / med / 1e3, 1))
        print("k_ekf_direct_update d=%d n=%d: median %.2f us (min %.2f, max %.2f) -> %.1f GB/s of 2 d^2 8 n bytes" % (d, n, med, reps.min(), reps.max(), byts / med / 1e3), flush=True)
        for s in ss:
            s.close()
ctx.close()

# ---- filter stage per frame, 192 streams in one lockstep group, frames 25..59 of the static lead-in: ZUPT firing vs off
syn = oracle_py.Synth(**DR.ZUPT_STREAM)
n_keys = syn.n_static + syn.n_loop
frames = np.zeros((2, n_keys, syn.h, syn.w), np.uint8)
for k in range(62):
    frames[0, k], frames[1, k] = syn.render(k)
imu = np.zeros(64 * 10 + 20, RN.IMU_SAMPLE)
for j in range(len(imu)):
    m = syn.imu(j)
    imu[j] = (m.time_stamp, tuple(m.angular_velocity), tuple(m.linear_acceleration))
fe, ekf = DR.small_cfgs()
N_STREAMS = 192
runs = {}
for name in ("on", "off"):
    run = RN.Runner(syn.calib, fe, ekf, n_groups=1, per_group=N_STREAMS)
    run.keep_trajectory(False)
    fb = syn.w * syn.h
    for i in range(N_STREAMS):
        run.set_sequence(i, frames.ctypes.data, frames.ctypes.data + n_keys * fb, 0, fb, syn.n_static, syn.n_loop, 1403715273262142976, 50000000, imu)
    if name == "on":
        run.set_zupt(True, max_disparity=DR.ZUPT_TEST_MAX_DISPARITY)
    run.run(0, 25, threaded=False)
    run.get_phases(reset=True)
    runs[name] = run
acc = {"on": {}, "off": {}}
frames_timed = 0
for k in range(25, 60, 5):
    for name in ("on", "off"):
        runs[name].run(k, 5, threaded=False)
        ph = runs[name].get_phases(reset=True)
        for p in RN.Runner.EKF_THREAD_PHASES:
            acc[name][p] = acc[name].get(p, 0.0) + ph[p]
    frames_timed += 5
for name in ("on", "off"):
    tot = sum(acc[name].values())
    out["filter_stage_" + name] = dict(ms_per_frame=round(tot * 1e3 / frames_timed, 3), phases_ms_per_frame={p: round(v * 1e3 / frames_timed, 3) for p, v in acc[name].items()},
                                       num_zupt_stream0=runs[name].num_zupt(0), num_zupt_last=runs[name].num_zupt(N_STREAMS - 1), state_dim=int(runs[name].cov(0).shape[0]))
    print("filter stage, %d streams, ZUPT %s: %.3f ms per frame; %s" % (N_STREAMS, name, tot * 1e3 / frames_timed, out["filter_stage_" + name]), flush=True)
if len(sys.argv) > 1:
    json.dump(out, open(sys.argv[1], "w"), indent=1)
for r in runs.values():
    r.close()
