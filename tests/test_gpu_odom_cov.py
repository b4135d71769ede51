"""GPU tests of the published odometry covariance (k_ekf_odom_cov behind mskf_ekf_get_odom_cov*, MsckfVio::publishCovariance,
Runner.odom_cov, the headless app's covariance file).

The expected value is always odom_cov_fixed (tests/odom_cov_reference.py: the arithmetic contract of DESIGN.md section 3) of
the covariance read back with mskf_ekf_get_cov, BIT FOR BIT (np.array_equal; -0 equals 0).  Every stream's T_imu_body rotation
is neither the identity nor symmetric: the synthetic calibration's identity would hide every transposition and ordering mistake.
"""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from msckf_stereo_c_amd import capi
from msckf_stereo_c_amd import runner as RN
from msckf_stereo_c_amd.ctypes_types import ODOM_COV, default_ekf_cfg, default_fe_cfg

import ekf_problems
import ekf_reference as R
import odom_cov_reference as OC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 21
ERR_INVALID = -1
W0 = H0 = 64                     # the smallest image a stream can be created with
MAX_CLONES = 4                   # ld = 48: d = 21, 27 (ld != d) and 45 (ld = d rounded up to a multiple of 8)
R_BODY = OC.rotation((1.0, 2.0, 3.0), 0.7)
CANARY = -777.25


def _stream(ctx, oracle, R_file=R_BODY):
    calib = oracle.euroc_calib(W0, H0)
    if R_file is not None:
        calib = OC.calib_with_imu_body(calib, R_file, t=(0.1, -0.2, 0.05))
    return capi.Stream(ctx, calib, default_fe_cfg(), default_ekf_cfg(max_cam_state_size=MAX_CLONES))


def _symmetric(d, rng):
    """Not a covariance to look at (indefinite, scales 1e-4 .. 1e1 per state), but exactly symmetric."""
    A = rng.normal(size=(d, d)) * np.outer(10.0 ** rng.uniform(-4, 1, size=d), 10.0 ** rng.uniform(-4, 1, size=d))
    return (A + A.T) / 2


def _expect(s):
    """odom_cov_fixed of the stream's covariance as mskf_ekf_get_cov returns it, as one 48-double row."""
    return OC.as_record(*OC.odom_cov_fixed(s.ekf_get_cov(), OC.body_rotation(s.calib)))


def _row(rec):
    return np.ascontiguousarray(rec).view(np.float64).reshape(-1, 48)


def _canary(n):
    out = np.zeros(n, ODOM_COV)
    out.view(np.float64)[:] = CANARY
    return out


# ------------------------------------------------------------------------------------------------ 3. single stream
@pytest.mark.parametrize("d", [21, 27, 21 + 6 * 4])
def test_odom_cov_single(gpu_ctx, oracle, d):
    """mskf_ekf_get_odom_cov on one stream: pose, twist and pos_var bitwise those of the contract; pos_var bitwise diag(P)[12:15];
    the same P behind the identity calibration returns the raw blocks bitwise."""
    rng = np.random.default_rng(300 + d)
    P = _symmetric(d, rng)
    assert np.array_equal(P, P.T)
    s, s_id = _stream(gpu_ctx, oracle), _stream(gpu_ctx, oracle, None)
    for x in (s, s_id):
        x.ekf_set_cov(P)
    got = s.ekf_odom_cov()
    Pb = s.ekf_get_cov()
    assert np.array_equal(Pb, P)
    pose, twist, pv = OC.odom_cov_fixed(Pb, OC.body_rotation(s.calib))
    assert np.array_equal(got["pose"], pose)
    assert np.array_equal(got["twist"], twist)
    assert np.array_equal(got["pos_var"], pv) and np.array_equal(got["pos_var"], np.diag(Pb)[12:15])
    assert not np.array_equal(got["pose"][0:3, 0:3], Pb[12:15, 12:15])           # the rotation did something
    raw = s_id.ekf_odom_cov()
    assert np.array_equal(OC.body_rotation(s_id.calib), np.eye(3))
    assert np.array_equal(raw["pose"][0:3, 0:3], Pb[12:15, 12:15]) and np.array_equal(raw["pose"][0:3, 3:6], Pb[12:15, 0:3])
    assert np.array_equal(raw["pose"][3:6, 0:3], Pb[0:3, 12:15]) and np.array_equal(raw["pose"][3:6, 3:6], Pb[0:3, 0:3])
    assert np.array_equal(raw["twist"], Pb[6:9, 6:9]) and np.array_equal(raw["pos_var"], np.diag(Pb)[12:15])
    for x in (s, s_id):
        x.close()


# ------------------------------------------------------------------------------------------------ 4. batches
@pytest.mark.parametrize("n", [1, 2, 3, 5])
def test_odom_cov_batch_equals_single_calls(gpu_ctx, oracle, n):
    """n streams in one launch: 48 n threads end inside a wavefront (48), past one (96), at a boundary (192 = 3 x 64) and past
    it (240).  Each stream has its own d, P and rotation; the batch equals the single calls and the contract bitwise, and the
    records of `out` beyond the n-th keep their canary."""
    rng = np.random.default_rng(400 + n)
    ss = []
    for i in range(n):
        s = _stream(gpu_ctx, oracle, OC.rotation(rng.normal(size=3), 0.5 + 0.4 * i))
        s.ekf_set_cov(_symmetric(N + 6 * ((i + n) % 5), rng))
        ss.append(s)
    want = np.array([_expect(s) for s in ss])
    single = np.array([_row(s.ekf_odom_cov())[0] for s in ss])
    assert np.array_equal(single, want)
    out = _canary(n + 2)
    gpu_ctx.ekf_odom_cov_batch_begin(ss, out=out)
    gpu_ctx.ekf_odom_cov_batch_end()
    assert np.array_equal(_row(out)[:n], single)
    assert (_row(out)[n:] == CANARY).all()
    assert np.array_equal(_row(gpu_ctx.ekf_odom_cov_batch(ss)), single)
    for s in ss:
        s.close()


# ------------------------------------------------------------------------------------------------ 5. stream order
def test_odom_cov_is_ordered_behind_the_filter(gpu_ctx, oracle):
    """predict_batch with augmentation -> update -> clone removal -> read-out, with no synchronisation from the test between
    the removal and the read-out: the result is that of the covariance the chain leaves, and the read-out leaves P as a twin
    stream that ran the same chain without a read-out has it."""
    calib = oracle.euroc_calib(W0, H0)
    rng = np.random.default_rng(51)
    P0 = R.spd(N + 6 * 3, rng)
    steps = R.imu_steps(5, 0.005, gyro=(0.0, 3.0, 0.0), q0=R.quat_axis_angle((1.0, 2.0, 3.0), 2.0), seed=5, jitter=0.05)
    J = R.augment_jacobian(rng)
    pr = ekf_problems.make_problem(calib, seed=8, n_clones=4, n_feat=12, min_obs=3)
    kw = dict(gravity=pr["gravity"], clones=pr["clones"], positions=pr["positions"], obs_start=pr["obs_start"],
              obs_clone=pr["obs_clone"], obs_z=pr["obs_z"], dof_offset=-1, apply_row_cap=True)
    s, twin = _stream(gpu_ctx, oracle), _stream(gpu_ctx, oracle)
    got = None
    for x in (s, twin):
        x.ekf_set_cov(P0)
        gpu_ctx.ekf_predict_batch([x], [steps], [J])
        assert x.ekf_update(**kw)["rows"] > 0
        gpu_ctx.ekf_remove_clones_batch([x], [(0, 2)])
        if x is s:
            got = _row(s.ekf_odom_cov())[0]
    P1 = s.ekf_get_cov()
    assert P1.shape == (N + 6 * 2,) * 2 and not np.array_equal(P1[:N, :N], P0[:N, :N])
    assert np.array_equal(got, OC.as_record(*OC.odom_cov_fixed(P1, OC.body_rotation(s.calib))))
    assert np.array_equal(P1, twin.ekf_get_cov())
    assert np.array_equal(_row(s.ekf_odom_cov())[0], got) and np.array_equal(s.ekf_get_cov(), P1)
    for x in (s, twin):
        x.close()


# ------------------------------------------------------------------------------------------------ 6. protocol
def _refused(fn, *needles):
    with pytest.raises(capi.MskfError) as e:
        fn()
    assert e.value.code == ERR_INVALID
    for needle in needles:
        assert needle in str(e.value), str(e.value)


def test_odom_cov_protocol(gpu_ctx, oracle):
    """The _begin / _end protocol of the position variances, on the record the two kinds of read-out share."""
    rng = np.random.default_rng(61)
    s = _stream(gpu_ctx, oracle)
    P0 = R.spd(N + 6 * 2, rng)
    s.ekf_set_cov(P0)
    steps = R.imu_steps(3, 0.005, gyro=(0.0, 3.0, 0.0), q0=R.quat_axis_angle((1.0, 2.0, 3.0), 2.0))
    J = R.augment_jacobian(rng)
    L = gpu_ctx.L
    L.mskf_ekf_get_odom_cov_batch_begin.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.c_void_p]
    L.mskf_ekf_get_odom_cov_batch.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.c_void_p]
    L.mskf_ekf_get_odom_cov.argtypes = [C.c_void_p, C.c_void_p]
    L.mskf_ekf_get_odom_cov_batch_end.argtypes = [C.c_void_p]
    # ---- refused arguments: nothing pending afterwards, the output untouched
    other = capi.Context(0)
    try:
        foreign = _stream(other, oracle)
        out = _canary(2)
        hs, hs_null, hs_foreign = capi._handles([s]), capi._handles([None]), capi._handles([s, foreign])
        po = out.ctypes.data_as(C.c_void_p)
        for f in (L.mskf_ekf_get_odom_cov_batch_begin, L.mskf_ekf_get_odom_cov_batch):
            assert f(None, 1, hs, po) == ERR_INVALID
            assert f(gpu_ctx.h, 1, None, po) == ERR_INVALID
            assert f(gpu_ctx.h, 1, hs, None) == ERR_INVALID
            assert f(gpu_ctx.h, 0, hs, po) == ERR_INVALID
            assert f(gpu_ctx.h, -1, hs, po) == ERR_INVALID
            assert f(gpu_ctx.h, 1, hs_null, po) == ERR_INVALID
            assert f(gpu_ctx.h, 2, hs_foreign, po) == ERR_INVALID
        assert L.mskf_ekf_get_odom_cov(None, po) == ERR_INVALID and L.mskf_ekf_get_odom_cov(s.h, None) == ERR_INVALID
        assert L.mskf_ekf_get_odom_cov_batch_end(None) == ERR_INVALID
        assert L.mskf_ekf_get_odom_cov_batch_end(gpu_ctx.h) == 0             # nothing pending: MSKF_OK
        assert (_row(out) == CANARY).all()
        assert np.array_equal(gpu_ctx.ekf_pos_var_batch([s])[0], np.diag(P0)[12:15])       # the arena is free
        foreign.close()
    finally:
        other.close()
    # ---- a pending covariance read-out owns the prediction arena
    name = ("read-out", "mskf_ekf_get_odom_cov_batch_end")
    out = gpu_ctx.ekf_odom_cov_batch_begin([s])
    try:
        _refused(lambda: gpu_ctx.ekf_predict_batch([s], [steps], [J]), *name)
        _refused(lambda: s.ekf_augment(J), *name)
        _refused(lambda: gpu_ctx.ekf_remove_clones_batch([s], [(0, 1)]), *name)
        _refused(lambda: gpu_ctx.ekf_pos_var_batch_begin([s]), *name)
        second = _canary(1)
        _refused(lambda: gpu_ctx.ekf_odom_cov_batch_begin([s], out=second), *name)
        assert (_row(second) == CANARY).all()
        _refused(gpu_ctx.ekf_pos_var_batch_end, *name)                  # the other kind's _end does not complete it
    finally:
        gpu_ctx.ekf_odom_cov_batch_end()
    gpu_ctx.ekf_odom_cov_batch_end()                                    # _end twice: MSKF_OK
    assert np.array_equal(_row(out)[0], OC.as_record(*OC.odom_cov_fixed(P0, OC.body_rotation(s.calib))))
    assert s.ekf_dim() == P0.shape[0] and np.array_equal(s.ekf_get_cov(), P0)
    # ---- after _end everything works again
    gpu_ctx.ekf_predict_batch([s], [steps], [J])
    assert s.ekf_dim() == P0.shape[0] + 6
    gpu_ctx.ekf_remove_clones_batch([s], [(0, 1)])
    assert s.ekf_dim() == P0.shape[0] - 6
    pv = gpu_ctx.ekf_pos_var_batch_begin([s])
    # ---- ... and a pending position-variance read-out refuses a covariance read-out the same way
    try:
        third = _canary(1)
        _refused(lambda: gpu_ctx.ekf_odom_cov_batch_begin([s], out=third), "read-out", "mskf_ekf_get_pos_var_batch_end")
        _refused(s.ekf_odom_cov, "read-out", "mskf_ekf_get_pos_var_batch_end")
        _refused(gpu_ctx.ekf_odom_cov_batch_end, "read-out", "mskf_ekf_get_pos_var_batch_end")
        assert (_row(third) == CANARY).all()
    finally:
        gpu_ctx.ekf_pos_var_batch_end()
    assert np.array_equal(pv[0], np.diag(s.ekf_get_cov())[12:15])
    assert np.array_equal(_row(gpu_ctx.ekf_odom_cov_batch([s]))[0], _expect(s))
    s.close()


# ------------------------------------------------------------------------------------------------ 7. runner
RUN_W, RUN_H, RUN_FRAMES = 188, 120, 36


def _small_fe():
    fe = default_fe_cfg()
    fe.det_rows, fe.det_cols = 15, 24
    return fe


def _attach(run, syns, n_frames, keep):
    for i, syn in enumerate(syns):
        n_keys = syn.n_static + syn.n_loop
        frames = np.empty((2, n_keys, syn.h, syn.w), np.uint8)
        for k in range(min(n_keys, n_frames + 1)):
            frames[0, k], frames[1, k] = syn.render(k)
        imu = np.zeros((n_frames + 3) * 10 + 20, RN.IMU_SAMPLE)
        for j in range(len(imu)):
            m = syn.imu(j)
            imu[j] = (m.time_stamp, tuple(m.angular_velocity), tuple(m.linear_acceleration))
        keep.append(frames)
        fb = syn.w * syn.h
        run.set_sequence(i, frames.ctypes.data, frames.ctypes.data + n_keys * fb, 0, fb, syn.n_static, syn.n_loop,
                         1403715273262142976, 50000000, imu)


def test_runner_publishes_covariances(oracle):
    """Runner.publish_covariance / Runner.odom_cov on two 188 x 120 streams over 36 frames (a 6-clone window: it fills, prunes and
    removes clones inside the run), trajectory kept, T_imu_body not the identity.
    (e) is measured against the oracle's covariance per frame, through the reference's literal H P H^T in long double, at the
    bar tests/test_gpu_system.py uses for cov() against the oracle: 1e-5 of the largest entry of the block compared."""
    fe, ekf = _small_fe(), default_ekf_cfg(max_cam_state_size=6)
    syns = [oracle.Synth(seed=0x5EED0090 + i, width=RUN_W, height=RUN_H, motion_scale=1.0 + 0.5 * i) for i in range(2)]
    calib = OC.calib_with_imu_body(syns[0].calib, R_BODY, t=(0.1, -0.2, 0.05))
    Rb = OC.body_rotation(calib)
    keep, runs = [], {}
    for name, cov_on, pipelined in (("lockstep", True, False), ("pipelined", True, True), ("off", False, False)):
        run = RN.Runner(calib, fe, ekf, 1, 2, host_threads=1)
        run.keep_trajectory(True)
        if cov_on:
            run.publish_covariance(True)
        _attach(run, syns, RUN_FRAMES, keep)
        run.run(0, RUN_FRAMES, threaded=True, pipelined=pipelined)
        runs[name] = run
    a, b, off = runs["lockstep"], runs["pipelined"], runs["off"]
    try:
        for s in range(2):
            poses, oc = a.poses(s), a.odom_cov(s)
            assert len(oc) == len(poses) > 8                                                    # (a)
            assert a.num_resets(s) == 0 and a.num_updates(s) > 0
            assert np.array_equal(_row(oc[-1:])[0], OC.as_record(*OC.odom_cov_fixed(a.cov(s), Rb)))       # (b)
            assert np.array_equal(_row(oc), _row(b.odom_cov(s)))                                # (c)
            assert all(np.array_equal(poses[f], b.poses(s)[f]) for f in ("t", "p", "q"))
            po = off.poses(s)                                                                   # (d)
            assert np.array_equal(poses["p"], po["p"]) and np.array_equal(poses["q"], po["q"]) and np.array_equal(poses["t"], po["t"])
            assert np.array_equal(a.dump(s)[0], off.dump(s)[0]) and np.array_equal(a.cov(s), off.cov(s))
            assert a.num_updates(s) == off.num_updates(s)
            assert len(off.odom_cov(s)) == 0                                                    # (f)
            # (e) the oracle, frame by frame
            osys = oracle.OracleSystem(calib, fe, ekf)
            lit = []

            def on_frame(k, o):
                if o.L.orc_system_num_poses(o.h) > len(lit):
                    lit.append(OC.odom_cov_literal(o.cov(), Rb))
            syns[s].feed(osys, RUN_FRAMES, on_frame)
            assert len(lit) == len(oc) and osys.num_resets() == 0
            worst = 0.0
            for rec, (lp, lt, lv) in zip(oc, lit):
                for got, ref in ((rec["pose"][0:3, 0:3], lp[0:3, 0:3]), (rec["pose"][0:3, 3:6], lp[0:3, 3:6]), (rec["pose"][3:6, 0:3], lp[3:6, 0:3]),
                                 (rec["pose"][3:6, 3:6], lp[3:6, 3:6]), (rec["twist"], lt), (rec["pos_var"], lv)):
                    ref = np.asarray(ref, dtype=np.float64)
                    if not ref.any():                       # (the cross blocks before the first update: exactly zero on both sides)
                        assert not got.any()
                        continue
                    worst = max(worst, float(np.abs(got - ref).max() / np.abs(ref).max()))
            print("stream %d: %d records, worst block difference to the oracle %.3e of the block's largest entry" % (s, len(oc), worst))
            assert worst < 1e-5
    finally:
        for r in runs.values():
            r.close()


# ------------------------------------------------------------------------------------------------ 8. headless app
def _app_time(ns):
    """run_euroc_single_thread's time stamp parsing: stoi(seconds) * 1e9 + stoi(nanoseconds) in double, then * 1e-9."""
    return (float(ns // 1000000000) * 1e9 + float(ns % 1000000000)) * 1e-9


def _write_mav0(tmp_path, syn, calib, n_frames):
    """A tiny EuRoC mav0 tree + config directory, laid out as tests/test_gpu_app.py lays out its own (that file builds its tree
    inside its test and offers nothing to import).  Returns (mav0, config dir, frame times, IMU samples as the app parses them)."""
    from PIL import Image
    mav0 = tmp_path / "mav0"
    for c in (0, 1):
        (mav0 / ("cam%d" % c) / "data").mkdir(parents=True)
    (mav0 / "imu0").mkdir()
    t0_ns, dt_ns = 1403715273262142976, 50000000
    rows = []
    for k in range(n_frames):
        a, b = syn.render(k)
        name = "%d.png" % (t0_ns + k * dt_ns)
        Image.fromarray(a).save(mav0 / "cam0" / "data" / name)
        Image.fromarray(b).save(mav0 / "cam1" / "data" / name)
        rows.append("%d,%s\r" % (t0_ns + k * dt_ns, name))
    for c in (0, 1):
        (mav0 / ("cam%d" % c) / "data.csv").write_text("#timestamp [ns],filename\r\n" + "\n".join(rows) + "\n")
    lines, imu = ["#timestamp [ns],w_x,w_y,w_z,a_x,a_y,a_z"], []
    for j in range((n_frames + 2) * 10):
        m = syn.imu(j)
        txt = ["%.9g" % v for v in list(m.angular_velocity) + list(m.linear_acceleration)]
        lines.append("%d,%s" % (t0_ns + j * (dt_ns // 10), ",".join(txt)))
        vals = [float(np.float32(float(x))) for x in txt]                    # std::stof
        imu.append((_app_time(t0_ns + j * (dt_ns // 10)), vals[:3], vals[3:]))
    (mav0 / "imu0" / "data.csv").write_text("\n".join(lines) + "\n")
    cfg = tmp_path / "config"
    shutil.copytree(os.path.join(ROOT, "config"), cfg)

    def mat(v):
        return "[" + ", ".join("%.17g" % x for x in v) + "]"
    cam = "  camera_model: pinhole\n  distortion_coeffs: %s\n  distortion_model: radtan\n  intrinsics: %s\n  resolution: [%d, %d]\n"
    (cfg / "camchain-imucam-euroc.yaml").write_text(
        "cam0:\n  T_cam_imu: %s\n" % mat(calib.T_cam0_imu) + cam % (mat(calib.cam0_distortion), mat(calib.cam0_intrinsics), syn.w, syn.h)
        + "cam1:\n  T_cn_cnm1: %s\n" % mat(calib.T_cam1_cam0) + cam % (mat(calib.cam1_distortion), mat(calib.cam1_intrinsics), syn.w, syn.h)
        + "T_imu_body: %s\n" % mat(calib.T_imu_body))
    return mav0, cfg, [_app_time(t0_ns + k * dt_ns) for k in range(n_frames)], imu


def _feed_like_the_app(run, syn, times, imu):
    """The frames of _write_mav0 through stream 0 of a Runner in the app's order: IMU samples up to the first one past the image."""
    from msckf_stereo_c_amd.ctypes_types import ImuSample
    j = 0
    for k, t_img in enumerate(times):
        while True:
            t, w, acc = imu[j]
            j += 1
            m = ImuSample()
            m.time_stamp = t
            m.angular_velocity[:] = w
            m.linear_acceleration[:] = acc
            run.imu(0, m)
            if not (t <= t_img):
                break
        a, b = syn.render(k)
        run.step([a], [b], [t_img])


def test_app_writes_the_covariance_file(tmp_path, oracle):
    """run_euroc_single_thread with `covariance_out: cov_out.txt` in app_msckfvio.yaml: one line per line of pose_out.txt with
    the same time stamps, 1 + 36 + 9 numbers each; the last line is the last record of a Runner fed the same files' content, to
    the six decimals the std::fixed stream format prints; pose_out.txt is byte for byte what the app writes without the option."""
    from msckf_stereo_c_amd import build
    build.build_all()
    n_frames = 32
    syn = oracle.Synth(seed=0x5EED0095, width=RUN_W, height=RUN_H, n_static=21, motion_scale=2.0)
    calib = OC.calib_with_imu_body(syn.calib, R_BODY, t=(0.1, -0.2, 0.05))
    mav0, cfg, times, imu = _write_mav0(tmp_path, syn, calib, n_frames)
    exe = os.path.join(ROOT, "msckf_stereo_c_amd", "_build", "run_euroc_single_thread")
    plain_yaml = (cfg / "app_msckfvio.yaml").read_text()
    outs = {}
    for name, yaml in (("off", plain_yaml), ("on", plain_yaml + "\ncovariance_out: cov_out.txt\n")):
        (cfg / "app_msckfvio.yaml").write_text(yaml)
        work = tmp_path / ("build_" + name)
        work.mkdir()
        res = subprocess.run([exe, str(mav0)], cwd=work, capture_output=True, text=True, timeout=120)
        assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
        outs[name] = work
    assert not (outs["off"] / "cov_out.txt").exists()
    assert (outs["on"] / "pose_out.txt").read_bytes() == (outs["off"] / "pose_out.txt").read_bytes()
    pose_lines = (outs["on"] / "pose_out.txt").read_text().splitlines()
    cov_lines = (outs["on"] / "cov_out.txt").read_text().splitlines()
    assert len(cov_lines) == len(pose_lines) > 5
    assert [l.split()[0] for l in cov_lines] == [l.split()[0] for l in pose_lines]
    assert all(len(l.split()) == 1 + 36 + 9 for l in cov_lines)
    assert all(len(v.split(".")[1]) == 6 for v in cov_lines[-1].split())          # the format of pose_out.txt (std::fixed, 6 decimals)
    # the same stream through a Runner (the app's default configuration: config/app_imgproc.yaml, app_msckfvio.yaml)
    run = RN.Runner(calib, default_fe_cfg(), default_ekf_cfg(), 1, 1)
    try:
        run.publish_covariance(True)
        _feed_like_the_app(run, syn, times, imu)
        oc = run.odom_cov(0)
        assert len(oc) == len(cov_lines)
        last = np.array([float(v) for v in cov_lines[-1].split()])
        assert abs(last[0] - run.poses(0)["t"][-1]) <= 1e-6
        want = _row(oc[-1:])[0][:45]
        assert np.abs(want).max() > 1e-4                                        # digits to compare survive the six decimals
        assert np.abs(last[1:] - want).max() <= 1e-6, np.abs(last[1:] - want).max()       # one unit of the last printed place
    finally:
        run.close()


def test_app_equals_a_runner_of_one_line_by_line(tmp_path, oracle):
    """The single-stream callbacks (System::stereo_callback / backend_callback, what the app runs) against a Runner(..., 1, 1) fed
    the same files' content: EVERY line of pose_out.txt and of the covariance file equals, as text, the Runner's record of the
    same frame printed "%.6f" per number (the app's std::fixed six decimals; both sides round correctly).
    42 frames, not 32: the camera stands still for 21 frames, the filter's first frame is frame 20 (200 IMU samples), and the
    app's window of 20 clones is full at frame 39 and again at frame 41, so the run has frames without an update (the variance
    read-out of its own), lost-feature updates, two pruning updates and two clone removals."""
    from msckf_stereo_c_amd import build
    build.build_all()
    n_frames = 42
    syn = oracle.Synth(seed=0x5EED0095, width=RUN_W, height=RUN_H, n_static=21, motion_scale=2.0)
    calib = OC.calib_with_imu_body(syn.calib, R_BODY, t=(0.1, -0.2, 0.05))
    mav0, cfg, times, imu = _write_mav0(tmp_path, syn, calib, n_frames)
    with open(cfg / "app_msckfvio.yaml", "a") as f:
        f.write("\ncovariance_out: cov_out.txt\n")
    work = tmp_path / "build"
    work.mkdir()
    exe = os.path.join(ROOT, "msckf_stereo_c_amd", "_build", "run_euroc_single_thread")
    res = subprocess.run([exe, str(mav0)], cwd=work, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    pose_lines = (work / "pose_out.txt").read_text().splitlines()
    cov_lines = (work / "cov_out.txt").read_text().splitlines()
    ekf = default_ekf_cfg()
    run = RN.Runner(calib, default_fe_cfg(), ekf, 1, 1)
    try:
        run.keep_trajectory(True)
        run.publish_covariance(True)
        _feed_like_the_app(run, syn, times, imu)
        poses, oc = run.poses(0), run.odom_cov(0)
        cap = ekf.max_cam_state_size
        print("poses %d, updates %d, clones %d of %d, resets %d" % (len(poses), run.num_updates(0), run.num_clones(0), cap, run.num_resets(0)))
        # the run reached every path of the filter's frame
        assert run.num_updates(0) > 0
        # a full window is pruned by two in the same frame: cap - 2 or cap - 1 clones after a frame, and at least `cap` filter frames
        assert len(poses) >= cap and run.num_clones(0) in (cap - 2, cap - 1)
        assert run.num_resets(0) == 0
        assert len(poses) > run.num_updates(0)               # some published frame had no update: its variances were fetched on their own
        fmt = lambda row: " ".join("%.6f" % v for v in row)
        assert len(pose_lines) == len(poses) and len(cov_lines) == len(oc) == len(poses)
        for k in range(len(poses)):
            assert pose_lines[k] == fmt([poses["t"][k]] + list(poses["p"][k]) + list(poses["q"][k])), k
            assert cov_lines[k] == fmt([poses["t"][k]] + list(_row(oc[k:k + 1])[0][:45])), k
    finally:
        run.close()
