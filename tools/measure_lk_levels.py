"""Times of the deeper LK pyramids on the device (DESIGN.md section 5 has one set of them): the C2 bench shape (752 x 480, 1536
streams in 8 batches of 192, about 437 points per stream), every stream at four levels (the default) and at six.  From the
contexts' HIP-event timing of one lockstep run each, every launch timed:

  * the track launch (MSKF_K_LK): k_track4 at four levels, k_track4_deep at six; milliseconds per launch.  A frame makes two of
    them (the previous grid's points, then the new candidates) over the 192 streams of a batch; the figure is the mean over both;
  * k_pyr_down_deep (the MSKF_K_PYR_DEEP slot): the levels 4 and 5 of both cameras of the 192 streams of a batch, one launch per
    frame; at four levels the slot counts nothing.

    python tools/measure_lk_levels.py [out.json]
"""
import json
import os
import sys

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
for levels in (4, 6):
    run = R.Runner(syns[0].calib, fe, ekf, args.groups, per_group)
    d_frames = synth_device.render_sequences(syns, n_keys, torch.device("cuda", 0), hip_stream=run.hip_stream(0))
    fb = args.width * args.height
    for s in range(args.streams):
        u = s % UNIQUE
        run.set_sequence(s, d_frames.data_ptr() + (u * 2 + 0) * n_keys * fb, d_frames.data_ptr() + (u * 2 + 1) * n_keys * fb, 2, fb, 25, args.loop,
                         bench.T0_NS, bench.FRAME_DT_NS, imus[u])
    run.keep_trajectory(False)
    if levels != 4:
        run.set_lk_levels(levels)
    run.run(0, PRIME, threaded=True)
    run.set_timing(1)
    run.get_timing(reset=True)
    run.run(PRIME, FRAMES, threaded=True)
    t = run.get_timing(reset=True)
    run.set_timing(False)
    lk_ms, lk_n, lk_units = t["k_track4"]
    g_ms, g_n, _ = t["k_pt_geom"]
    n_feat = [len(run.dump(g * per_group)[0]) for g in range(args.groups)]
    rec = dict(track_ms_per_launch=round(lk_ms / lk_n, 4), track_launches=lk_n, point_tracks_per_stream_per_launch=round(lk_units / lk_n / per_group, 1),
               deep_pyramid_launches=g_n, features_stream0_of_each_batch=n_feat)
    if g_n:
        rec["k_pyr_down_deep_ms_per_launch"] = round(g_ms / g_n, 4)
    out["levels_%d" % levels] = rec
    print("lk levels %d: %s" % (levels, rec), flush=True)
    run.close()
    del d_frames
if len(sys.argv) > 1:
    json.dump(out, open(sys.argv[1], "w"), indent=1)
