"""Times of the extended instantiation of the track kernel on the device (DESIGN.md section 5 has one set of them): the C2 bench
shape (752 x 480, 1536 streams in 8 batches of 192, about 437 points per stream), the same radtan lens through both launches.
From the contexts' HIP-event timing of one lockstep run each, every launch timed (the MSKF_K_LK slot):

  * base: no stream has an extended model, every track launch is k_track4;
  * extended: every camera is set to radtan8 with the calibration's k1 k2 p1 p2 and k3 = .. = k6 = 0, so every track launch is
    k_track4_ext and computes the same bits (the run's features are compared).

A frame makes two launches (the previous grid's points, then the new candidates), over the 192 streams of a batch; the figures
are means over both.

    python tools/measure_camera_models.py [out.json]
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench                                                # noqa: E402

PRIME, FRAMES, UNIQUE = 40, 30, 8

args = bench.parse(["--config", "c2", "--unique", str(UNIQUE)])
import torch                                                # noqa: E402
from msckf_stereo_c_amd import runner as R                  # noqa: E402
from msckf_stereo_c_amd import synth_device                 # noqa: E402
oracle_py = bench.build_libraries()
fe, ekf = bench.make_cfgs(args)
per_group = args.streams // args.groups
n_keys = 25 + args.loop
syns = bench.make_generators(oracle_py, args, 0, 1)
imus = [bench.imu_array(s, (PRIME + FRAMES + 3) * 10 + 20) for s in syns]
out = {"shape": dict(width=args.width, height=args.height, streams=args.streams, batches=args.groups, streams_per_launch=per_group, grid=args.grid,
                     frames_timed=FRAMES)}
dumps = {}
for name in ("base", "extended"):
    run = R.Runner(syns[0].calib, fe, ekf, args.groups, per_group)
    d_frames = synth_device.render_sequences(syns, n_keys, torch.device("cuda", 0), hip_stream=run.hip_stream(0))
    fb = args.width * args.height
    for s in range(args.streams):
        u = s % UNIQUE
        run.set_sequence(s, d_frames.data_ptr() + (u * 2 + 0) * n_keys * fb, d_frames.data_ptr() + (u * 2 + 1) * n_keys * fb, 2, fb, 25, args.loop,
                         bench.T0_NS, bench.FRAME_DT_NS, imus[u])
    run.keep_trajectory(False)
    if name == "extended":
        run.set_camera_model(0, "radtan8", list(syns[0].calib.cam0_distortion) + [0.0] * 4)
        run.set_camera_model(1, "radtan8", list(syns[0].calib.cam1_distortion) + [0.0] * 4)
    run.run(0, PRIME, threaded=True)
    run.set_timing(1)
    run.get_timing(reset=True)
    run.run(PRIME, FRAMES, threaded=True)
    t = run.get_timing(reset=True)
    run.set_timing(False)
    lk_ms, lk_n, lk_units = t["k_track4"]
    dumps[name] = [run.dump(g * per_group)[:4] for g in range(args.groups)]
    rec = dict(track_ms_per_launch=round(lk_ms / lk_n, 4), track_launches=lk_n, point_tracks_per_stream_per_launch=round(lk_units / lk_n / per_group, 1),
               features_stream0_of_each_batch=[len(d[0]) for d in dumps[name]])
    out[name] = rec
    print("track launch, %s: %s" % (name, rec), flush=True)
    run.close()
    del d_frames
out["same_features"] = all(np.array_equal(x, y) for a, b in zip(dumps["base"], dumps["extended"]) for x, y in zip(a, b))
out["extended_over_base"] = round(out["extended"]["track_ms_per_launch"] / out["base"]["track_ms_per_launch"], 3)
print("same features: %s, extended / base: %s" % (out["same_features"], out["extended_over_base"]), flush=True)
if len(sys.argv) > 1:
    json.dump(out, open(sys.argv[1], "w"), indent=1)
