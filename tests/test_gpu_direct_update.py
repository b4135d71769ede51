"""GPU tests of the direct measurement update (k_ekf_direct_update behind mskf_ekf_update_direct*, MsckfVio::queueVelocity /
queuePosition and the zero-velocity update behind Runner.fuse_velocity / fuse_position / set_zupt, the headless app's keys).

The expected value is always direct_update_fixed (tests/direct_update_reference.py: the arithmetic contract of DESIGN.md
section 3) of the covariance read back with mskf_ekf_get_cov, BIT FOR BIT (np.array_equal; -0 equals 0): P, delta_x, gamma and
the position variances.  tests/test_direct_update_reference.py shows on the CPU what that restatement is worth.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from msckf_stereo_c_amd import capi
from msckf_stereo_c_amd import runner as RN
from msckf_stereo_c_amd.ctypes_types import Calib, EkfCfg, EkfDirectArgs, FeCfg, ImuSample, default_ekf_cfg, default_fe_cfg

import direct_update_reference as DR
import ekf_problems
import ekf_reference as ER

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 21
ERR_INVALID = -1
W0 = H0 = 64                     # the smallest image a stream can be created with
CANARY = -777.25


def _stream(ctx, oracle, max_clones=64):
    return capi.Stream(ctx, oracle.euroc_calib(W0, H0), default_fe_cfg(), default_ekf_cfg(max_cam_state_size=max_clones))


def _max_clones(d):
    return max(4, (d - N) // 6)           # ld = d rounded up to 8: 24 (d = 21 .. 45), 64, 72, 208, 408


def _grow_on_device(ctx, s, d):
    """P grown by real predict / augment calls on the device, from DR.grow_inputs."""
    P0, seq = DR.grow_inputs(d)
    s.ekf_reset(P0)
    for steps, J in seq:
        ctx.ekf_predict_batch([s], [steps], [J])
    assert s.ekf_dim() == d
    return s.ekf_get_cov()


def _load(ctx, s, kind, d):
    if kind == "grown":
        return _grow_on_device(ctx, s, d)
    P = DR.make_P(kind, d)
    s.ekf_set_cov(P)
    return P


def _same(res, want):
    """The four outputs of a call against the restatement's, bitwise."""
    assert res["status"] == want["status"]
    assert np.array_equal(res["delta_x"], want["dx"])
    assert res["gamma"] == want["gamma"]
    assert np.array_equal(res["pos_var"], want["pos_var"])


# ------------------------------------------------------------------------------------------------ 1. bitwise
@pytest.mark.parametrize("kind", DR.P_KINDS)
@pytest.mark.parametrize("d", DR.DIMS)
def test_direct_update_bitwise(gpu_ctx, oracle, d, kind):
    """m = 1, 3, 6 with a dense and a selector H on each P of the set: P, delta_x, gamma and pos_var_out bitwise those of the
    contract, P == P.T bitwise, pos_var_out == diag(P)[12:15].  d = 21 (no clone), 27 (one), 63 / 69 (either side of 64: two and
    three 32-wide tiles), 201 (the bench's 30 clones), 405 (the 64-clone maximum, ld = 408)."""
    s = _stream(gpu_ctx, oracle, _max_clones(d))
    P0 = _load(gpu_ctx, s, kind, d)
    assert np.array_equal(P0, P0.T) and P0.shape == (d, d)
    for m in DR.ROWS:
        for dense in (True, False):
            rng = np.random.default_rng(d * 100 + m * 2 + dense)
            H, r, R = DR.make_measurement(P0, m, dense, rng, first_col=12 if m == 3 else 6)
            s.ekf_set_cov(P0)
            want = DR.direct_update_fixed(P0, H, r, R)
            assert want["status"] == 1
            res = s.ekf_update_direct(H, r, R)
            _same(res, want)
            P1 = s.ekf_get_cov()
            assert np.array_equal(P1, want["P"])
            assert np.array_equal(P1, P1.T)
            assert np.array_equal(res["pos_var"], np.diag(P1)[12:15])
            assert not np.array_equal(P1, P0)
    s.close()


# ------------------------------------------------------------------------------------------------ 2. gate and factorisation
def test_direct_update_gate_and_factorisation(gpu_ctx, oracle):
    d = 69
    s = _stream(gpu_ctx, oracle, _max_clones(d))
    P0 = DR.make_P("spd", d)
    rng = np.random.default_rng(2)
    H, r, R = DR.make_measurement(P0, 3, True, rng)
    applied = DR.direct_update_fixed(P0, H, r, R)
    gamma = applied["gamma"]
    assert gamma > 0
    # gamma above the gate: status 0, P bitwise unchanged, delta_x all zero, gamma and the (unchanged) variances reported
    for gate in (np.nextafter(gamma, 0.0), gamma / 2, 1e-300):
        s.ekf_set_cov(P0)
        res = s.ekf_update_direct(H, r, R, gate=gate)
        assert res["status"] == 0 and res["gamma"] == gamma
        assert not res["delta_x"].any()
        assert np.array_equal(res["pos_var"], np.diag(P0)[12:15])
        assert np.array_equal(s.ekf_get_cov(), P0)
        _same(res, DR.direct_update_fixed(P0, H, r, R, gate=gate))
    # gamma at or below the gate, and no gate (<= 0): applied
    for gate in (gamma, 2 * gamma, np.inf, 0.0, -1.0):
        s.ekf_set_cov(P0)
        res = s.ekf_update_direct(H, r, R, gate=gate)
        _same(res, applied)
        assert np.array_equal(s.ekf_get_cov(), applied["P"])
    # an indefinite P: S = H P H^T + R has a non-positive pivot (first, then second); status 2, P unchanged: arithmetic, not a fault
    Hs = np.zeros((2, N))
    Hs[0, 6] = Hs[1, 7] = 1.0
    for Pbad in (-np.eye(d), np.diag([1.0] * 7 + [-1.0] * (d - 7))):
        s.ekf_set_cov(Pbad)
        res = s.ekf_update_direct(Hs, [0.1, 0.2], 0.25 * np.eye(2))
        assert res["status"] == 2 and res["gamma"] == 0.0 and not res["delta_x"].any()
        assert np.array_equal(res["pos_var"], np.diag(Pbad)[12:15])
        assert np.array_equal(s.ekf_get_cov(), Pbad)
        _same(res, DR.direct_update_fixed(Pbad, Hs, [0.1, 0.2], 0.25 * np.eye(2)))
    s.close()


# ------------------------------------------------------------------------------------------------ 3. batches
def _case(i, d):
    """(P, problem or None) of stream i of a batch: its own P kind, row count and H kind; some streams sit out."""
    P = DR.make_P(("spd", "identity")[i % 2], d, seed=i)
    m = (3, 0, 6, 1, 0, 2)[i % 6]
    if m == 0:
        return P, None
    H, r, R = DR.make_measurement(P, m, i % 3 != 0, np.random.default_rng(50 + i))
    return P, dict(H=H, r=r, R=R, gate=0.0 if i % 2 else 1e6)


@pytest.mark.parametrize("n", [1, 2, 3, 5])
def test_direct_update_batch_equals_single_calls(gpu_ctx, oracle, n):
    """Batches of mixed d and m equal the single calls (and the contract) bitwise; streams with m = 0 inside a batch are bitwise
    untouched and report status 0, zero delta_x, gamma 0 and no variance (-1)."""
    dims = [(405, 27, 69, 21, 201)[(i + n) % 5] for i in range(n)]
    ss = [_stream(gpu_ctx, oracle, _max_clones(d)) for d in dims]
    twins = [_stream(gpu_ctx, oracle, _max_clones(d)) for d in dims]
    cases = [_case(i + n - 1, d) for i, d in enumerate(dims)]
    if n > 1:
        assert any(pr is None for _, pr in cases) and any(pr is not None for _, pr in cases)
    single = []
    for s, t, (P, pr) in zip(ss, twins, cases):
        s.ekf_set_cov(P)
        t.ekf_set_cov(P)
        single.append(None if pr is None else t.ekf_update_direct(**pr))
    got = gpu_ctx.ekf_update_direct_batch(ss, [pr for _, pr in cases])
    for s, t, (P, pr), one, res in zip(ss, twins, cases, single, got):
        if pr is None:
            assert res["status"] == 0 and res["gamma"] == 0.0 and not res["delta_x"].any() and (res["pos_var"] == -1.0).all()
            assert np.array_equal(s.ekf_get_cov(), P)
            continue
        want = DR.direct_update_fixed(P, pr["H"], pr["r"], pr["R"], pr["gate"])
        _same(one, want)
        _same(res, want)
        assert np.array_equal(s.ekf_get_cov(), want["P"]) and np.array_equal(t.ekf_get_cov(), want["P"])
    for s in ss + twins:
        s.close()


def test_direct_update_small_stream_beside_large(gpu_ctx, oracle):
    """A 27-dimensional stream gives the same bits alone and beside a 405-dimensional one (in either order)."""
    small, big = _stream(gpu_ctx, oracle, 4), _stream(gpu_ctx, oracle, 64)
    Ps, Pb = DR.make_P("spd", 27), DR.make_P("spd", 405)
    ms = DR.make_measurement(Ps, 3, True, np.random.default_rng(5))
    mb = DR.make_measurement(Pb, 6, True, np.random.default_rng(6))
    prs, prb = dict(H=ms[0], r=ms[1], R=ms[2]), dict(H=mb[0], r=mb[1], R=mb[2])
    small.ekf_set_cov(Ps)
    alone = small.ekf_update_direct(**prs)
    P_alone = small.ekf_get_cov()
    for order in ((small, big), (big, small)):
        small.ekf_set_cov(Ps)
        big.ekf_set_cov(Pb)
        res = gpu_ctx.ekf_update_direct_batch(list(order), [prs if x is small else prb for x in order])
        mine = res[order.index(small)]
        _same(mine, dict(status=alone["status"], dx=alone["delta_x"], gamma=alone["gamma"], pos_var=alone["pos_var"]))
        assert np.array_equal(small.ekf_get_cov(), P_alone)
        assert np.array_equal(big.ekf_get_cov(), DR.direct_update_fixed(Pb, *mb)["P"])
    small.close()
    big.close()


# ------------------------------------------------------------------------------------------------ 4. protocol
def _refused(fn, *needles):
    with pytest.raises(capi.MskfError) as e:
        fn()
    assert e.value.code == ERR_INVALID
    for needle in needles:
        assert needle in str(e.value), str(e.value)


def _feature_problem(calib):
    pr = ekf_problems.make_problem(calib, seed=8, n_clones=4, n_feat=12, min_obs=3)
    return dict(gravity=pr["gravity"], clones=pr["clones"], positions=pr["positions"], obs_start=pr["obs_start"],
                obs_clone=pr["obs_clone"], obs_z=pr["obs_z"], dof_offset=-1, apply_row_cap=True)


def test_direct_update_protocol(gpu_ctx, oracle):
    """The two kinds of update share one pending slot, each refusal names the pending call; a pending read-out refuses a direct
    update; a finished direct update leaves the stream as set_cov of the expected P does."""
    L = gpu_ctx.L
    L.mskf_ekf_update_batch_begin.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(capi.EkfUpdateArgs)]
    L.mskf_ekf_update_batch_end.argtypes = [C.c_void_p]
    rng = np.random.default_rng(41)
    d = N + 6 * 4
    s, twin = _stream(gpu_ctx, oracle, 4), _stream(gpu_ctx, oracle, 4)
    P0 = ER.spd(d, rng)
    H, r, R = DR.make_measurement(P0, 3, False, rng, first_col=12)
    direct = dict(H=H, r=r, R=R)
    kw = _feature_problem(s.calib)
    s.ekf_set_cov(P0)
    # ---- a pending feature update refuses a direct update (_begin, the batch call, the single call) and the direct _end
    fa, _keep, feat_result = capi.Stream._update_args(**kw)
    hs = capi._handles([s])
    assert L.mskf_ekf_update_batch_begin(gpu_ctx.h, 1, hs, C.byref(fa)) == 0
    try:
        name = ("an update batch", "mskf_ekf_update_batch_end")
        _refused(lambda: gpu_ctx.ekf_update_direct_batch_begin([s], [direct]), *name)
        _refused(lambda: s.ekf_update_direct(**direct), *name)
        _refused(gpu_ctx.ekf_update_direct_batch_end, *name)
    finally:
        assert L.mskf_ekf_update_batch_end(gpu_ctx.h) == 0
    assert feat_result()["rows"] > 0
    P1 = s.ekf_get_cov()
    # ---- a pending direct update refuses a feature update (_begin, the batch call) and the feature _end
    res = gpu_ctx.ekf_update_direct_batch_begin([s], [direct])[0]
    try:
        name = ("a direct update batch", "mskf_ekf_update_direct_batch_end")
        _refused(lambda: s.ekf_update(**kw), *name)
        _refused(lambda: capi._chk(L.mskf_ekf_update_batch_begin(gpu_ctx.h, 1, hs, C.byref(fa))), *name)
        _refused(lambda: capi._chk(L.mskf_ekf_update_batch_end(gpu_ctx.h)), *name)
        _refused(lambda: gpu_ctx.ekf_update_direct_batch_begin([s], [direct]), *name)
    finally:
        gpu_ctx.ekf_update_direct_batch_end()
    gpu_ctx.ekf_update_direct_batch_end()                                # _end twice: MSKF_OK
    want = DR.direct_update_fixed(P1, H, r, R)
    _same(res, want)
    assert np.array_equal(s.ekf_get_cov(), want["P"])
    # ---- a pending read-out refuses a direct update
    pv = gpu_ctx.ekf_pos_var_batch_begin([s])
    try:
        _refused(lambda: gpu_ctx.ekf_update_direct_batch_begin([s], [direct]), "read-out", "mskf_ekf_get_pos_var_batch_end")
    finally:
        gpu_ctx.ekf_pos_var_batch_end()
    assert np.array_equal(pv[0], np.diag(want["P"])[12:15])
    assert np.array_equal(s.ekf_get_cov(), want["P"])
    # ---- after _end: predict, feature update and clone removal give what they give after set_cov of the expected P
    twin.ekf_set_cov(want["P"])
    steps = ER.imu_steps(3, 0.005, gyro=(0.0, 3.0, 0.0), q0=ER.quat_axis_angle((1.0, 2.0, 3.0), 2.0))
    outs = []
    for x in (s, twin):
        gpu_ctx.ekf_remove_clones_batch([x], [(1, -1)])
        gpu_ctx.ekf_predict_batch([x], [steps], [ER.augment_jacobian(np.random.default_rng(9))])
        outs.append(x.ekf_update(**kw))
        assert outs[-1]["rows"] > 0
    assert np.array_equal(outs[0]["delta_x"], outs[1]["delta_x"]) and np.array_equal(outs[0]["gamma"], outs[1]["gamma"])
    assert np.array_equal(s.ekf_get_cov(), twin.ekf_get_cov())
    s.close()
    twin.close()


def _raw_args(m, H, r, R, dx, gate=0.0, pv=None):
    a = EkfDirectArgs()
    a.m, a.status, a.gamma, a.gate = m, 77, CANARY, gate
    a.H, a.r, a.R = (None if x is None else x.ctypes.data for x in (H, r, R))
    a.delta_x = None if dx is None else dx.ctypes.data
    a.pos_var_out = None if pv is None else pv.ctypes.data
    return a


def test_direct_update_refuses_invalid_arguments(gpu_ctx, oracle):
    """m outside 0..6, null pointers with m > 0, non-finite H / r / R, a NaN gate, R not symmetric or with a non-positive
    diagonal: MSKF_ERR_INVALID, outputs untouched (canaries), P unchanged, nothing pending: also for the LAST stream of a batch
    whose first is valid."""
    L = gpu_ctx.L
    L.mskf_ekf_update_direct.argtypes = [C.c_void_p, C.POINTER(EkfDirectArgs)]
    L.mskf_ekf_update_direct_batch.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(EkfDirectArgs)]
    L.mskf_ekf_update_direct_batch_begin.argtypes = L.mskf_ekf_update_direct_batch.argtypes
    d = 27
    s, first = _stream(gpu_ctx, oracle, 4), _stream(gpu_ctx, oracle, 4)
    P0 = DR.make_P("spd", d)
    s.ekf_set_cov(P0)
    first.ekf_set_cov(P0)
    rng = np.random.default_rng(3)
    H, r, R = DR.make_measurement(P0, 3, True, rng)
    H6, r6, R6 = DR.make_measurement(P0, 6, True, rng)

    def bad(x, idx, v):
        y = x.copy()
        y[idx] = v
        return y
    Rasym = bad(R, (0, 1), R[0, 1] * (1 + 1e-15))
    assert Rasym[0, 1] != Rasym[1, 0]
    dx = np.full(d, CANARY)
    pv = np.full(3, CANARY)
    cases = {
        "m = -1": _raw_args(-1, H, r, R, dx, pv=pv), "m = 7": _raw_args(7, H6, r6, R6, dx, pv=pv),
        "H null": _raw_args(3, None, r, R, dx, pv=pv), "r null": _raw_args(3, H, None, R, dx, pv=pv),
        "R null": _raw_args(3, H, r, None, dx, pv=pv), "delta_x null": _raw_args(3, H, r, R, None, pv=pv),
        "NaN in H": _raw_args(3, bad(H, (2, 20), np.nan), r, R, dx, pv=pv), "inf in H": _raw_args(3, bad(H, (0, 0), np.inf), r, R, dx, pv=pv),
        "NaN in r": _raw_args(3, H, bad(r, 2, np.nan), R, dx, pv=pv), "-inf in r": _raw_args(3, H, bad(r, 0, -np.inf), R, dx, pv=pv),
        "NaN in R": _raw_args(3, H, r, bad(bad(R, (1, 2), np.nan), (2, 1), np.nan), dx, pv=pv),
        "inf on R's diagonal": _raw_args(3, H, r, bad(R, (2, 2), np.inf), dx, pv=pv),
        "NaN gate": _raw_args(3, H, r, R, dx, gate=np.nan, pv=pv),
        "R not symmetric": _raw_args(3, H, r, Rasym, dx, pv=pv),
        "R zero diagonal": _raw_args(3, H, r, bad(R, (1, 1), 0.0), dx, pv=pv),
        "R negative diagonal": _raw_args(3, H, r, bad(R, (2, 2), -R[2, 2]), dx, pv=pv),
    }
    keep = []
    for name, a in cases.items():
        assert L.mskf_ekf_update_direct(s.h, C.byref(a)) == ERR_INVALID, name
        # ... and as the last stream of a batch behind a valid one: the valid stream is not touched either
        dx_first = np.full(d, CANARY)
        pair = (EkfDirectArgs * 2)(_raw_args(3, H, r, R, dx_first), a)
        keep.append(pair)
        for f in (L.mskf_ekf_update_direct_batch, L.mskf_ekf_update_direct_batch_begin):
            assert f(gpu_ctx.h, 2, capi._handles([first, s]), pair) == ERR_INVALID, name
        assert all(x.status == 77 and x.gamma == CANARY for x in (a, pair[0], pair[1])), name
        assert (dx == CANARY).all() and (pv == CANARY).all() and (dx_first == CANARY).all(), name
    ok = _raw_args(3, H, r, R, dx)
    # the same stream twice with rows (two workgroups on one P): refused; once with rows and once without: fine
    twice = (EkfDirectArgs * 2)(ok, _raw_args(1, H6, r6, R6[:1, :1].copy(), np.full(d, CANARY)))
    assert L.mskf_ekf_update_direct_batch(gpu_ctx.h, 2, capi._handles([s, s]), twice) == ERR_INVALID
    assert twice[0].status == 77 and (dx == CANARY).all() and np.array_equal(s.ekf_get_cov(), P0)
    hs = capi._handles([s])
    other = capi.Context(0)
    try:
        foreign = _stream(other, oracle, 4)
        for f in (L.mskf_ekf_update_direct_batch, L.mskf_ekf_update_direct_batch_begin):
            assert f(None, 1, hs, C.byref(ok)) == ERR_INVALID
            assert f(gpu_ctx.h, 0, hs, C.byref(ok)) == ERR_INVALID
            assert f(gpu_ctx.h, 1, None, C.byref(ok)) == ERR_INVALID
            assert f(gpu_ctx.h, 1, hs, None) == ERR_INVALID
            assert f(gpu_ctx.h, 1, capi._handles([None]), C.byref(ok)) == ERR_INVALID
            assert f(gpu_ctx.h, 1, capi._handles([foreign]), C.byref(ok)) == ERR_INVALID
        foreign.close()
    finally:
        other.close()
    assert L.mskf_ekf_update_direct(None, C.byref(ok)) == ERR_INVALID and L.mskf_ekf_update_direct(s.h, None) == ERR_INVALID
    assert (dx == CANARY).all()
    assert np.array_equal(s.ekf_get_cov(), P0) and np.array_equal(first.ekf_get_cov(), P0)
    # nothing is pending and the arenas are free: the valid call goes through
    gpu_ctx.ekf_update_direct_batch_end()
    want = DR.direct_update_fixed(P0, H, r, R)
    _same(s.ekf_update_direct(H, r, R), want)
    assert np.array_equal(s.ekf_get_cov(), want["P"])
    s.close()
    first.close()


# ------------------------------------------------------------------------------------------------ 5. runner, exact
T0_NS, DT_NS = 1403715273262142976, 50000000
CHI2_95_DOF3 = 7.8147279032511792          # include/mskf_chi2_table.h, mskf_chi2_ppf95[2]
RUN_FRAMES = 80


@pytest.fixture(scope="module")
def zupt_stream(oracle):
    """The separation test's stream, rendered once: (synth, frames (2, keys, h, w), IMU samples)."""
    syn = oracle.Synth(**DR.ZUPT_STREAM)
    n_keys = syn.n_static + syn.n_loop
    frames = np.zeros((2, n_keys, syn.h, syn.w), np.uint8)
    for k in range(RUN_FRAMES + 1):
        frames[0, k], frames[1, k] = syn.render(k)
    imu = np.zeros((RUN_FRAMES + 3) * 10 + 20, RN.IMU_SAMPLE)
    for j in range(len(imu)):
        m = syn.imu(j)
        imu[j] = (m.time_stamp, tuple(m.angular_velocity), tuple(m.linear_acceleration))
    return syn, frames, imu


def _runner(zupt_stream, n=1):
    syn, frames, imu = zupt_stream
    fe, ekf = DR.small_cfgs()
    run = RN.Runner(syn.calib, fe, ekf, n_groups=1, per_group=n)
    fb = syn.w * syn.h
    for i in range(n):
        run.set_sequence(i, frames.ctypes.data, frames.ctypes.data + frames.shape[1] * fb, 0, fb, syn.n_static, syn.n_loop, T0_NS, DT_NS, imu)
    return run


def _frame_time(k):
    ns = T0_NS + k * DT_NS
    return (float(ns // 1000000000) * 1e9 + float(ns % 1000000000)) * 1e-9


def _selector(first_col):
    H = np.zeros((3, N))
    H[np.arange(3), first_col + np.arange(3)] = 1.0
    return H


def _state_plus(state, dx):
    """Position and velocity of a 28-double IMU state after the correction dx (the other entries are not sums)."""
    return state[4:7] + dx[12:15], state[7:10] + dx[6:9]


def test_runner_fuses_position_and_velocity_exactly(zupt_stream):
    """A plain twin and a Runner of two streams in lockstep up to a moving frame K; there stream 0 fuses the twin's position +
    (0.01, 0, 0), stream 1 the twin's velocity + (0, 0.02, 0), cov 1e-4 I, ungated.  After that frame cov() is bitwise the
    restatement applied to the twin's cov(), position and velocity are the twin's + delta_x, the frame's published pose carries
    the correction, num_direct_updates == 1; a frame later nothing more is applied."""
    K = 70
    twin, other = _runner(zupt_stream), _runner(zupt_stream, 2)
    twin.run(0, K + 1, threaded=False)
    other.run(0, K, threaded=False)
    st, P = twin.imu_state(), twin.cov()
    assert np.abs(twin.poses()["p"][-1] - st[4:7]).max() < 1e-12      # the synthetic T_imu_body is the identity: pose = IMU position
    Rm = 1e-4 * np.eye(3)
    zp, zv = st[4:7] + np.array([0.01, 0.0, 0.0]), st[7:10] + np.array([0.0, 0.02, 0.0])
    t = _frame_time(K) - 0.025                                        # between frames K - 1 and K: frame K is the first with a stamp >= t
    other.fuse_position(0, t, zp, Rm, gated=False)
    other.fuse_velocity(1, t, zv, Rm, gated=False)
    assert other.num_direct_updates(0) == other.num_direct_updates(1) == 0
    other.run(K, 1, threaded=False)
    for i, (col, z) in enumerate(((12, zp), (6, zv))):
        x0 = st[4:7] if col == 12 else st[7:10]
        want = DR.direct_update_fixed(P, _selector(col), z - x0, Rm)
        assert want["status"] == 1 and np.abs(want["dx"][col:col + 3]).max() > 1e-3
        assert np.array_equal(other.cov(i), want["P"])
        got = other.imu_state(i)
        p, v = _state_plus(st, want["dx"])
        assert np.array_equal(got[4:7], p) and np.array_equal(got[7:10], v)
        assert np.abs(other.poses(i)["p"][-1] - got[4:7]).max() < 1e-12                      # the frame's pose carries the correction
        if col == 12:
            assert np.abs(other.poses(i)["p"][-1] - twin.poses()["p"][-1]).max() > 1e-3
        assert len(other.poses(i)) == len(twin.poses()) and other.poses(i)["t"][-1] == twin.poses()["t"][-1]
        assert np.array_equal(other.poses(i)[:-1], twin.poses()[:-1])
        assert other.num_direct_updates(i) == 1 and other.num_zupt(i) == 0
        assert other.num_updates(i) == twin.num_updates()
    other.run(K + 1, 1, threaded=False)
    assert other.num_direct_updates(0) == other.num_direct_updates(1) == 1
    assert other.num_resets(0) == other.num_resets(1) == 0
    # refused measurements raise and queue nothing
    for bad in (np.array([[1.0, 0.1, 0], [0.2, 1.0, 0], [0, 0, 1.0]]), np.diag([1.0, 0.0, 1.0]), np.full((3, 3), np.nan)):
        with pytest.raises(RN.MskfError):
            other.fuse_position(0, t, zp, bad)
    with pytest.raises(RN.MskfError):
        other.fuse_velocity(0, t, [np.inf, 0, 0], Rm)
    other.run(K + 2, 1, threaded=False)
    assert other.num_direct_updates(0) == 1
    twin.close()
    other.close()


# ------------------------------------------------------------------------------------------------ 6. zero-velocity run
def test_zupt_run(zupt_stream):
    """The separation test's stream and threshold, 80 frames, frame by frame with the zero-velocity update on and off, once more
    on in a pipelined run, and through a Runner that never heard of the feature."""
    on, off, plain, piped = (_runner(zupt_stream) for _ in range(4))
    on.set_zupt(True, max_disparity=DR.ZUPT_TEST_MAX_DISPARITY)
    piped.set_zupt(True, max_disparity=DR.ZUPT_TEST_MAX_DISPARITY)
    off.set_zupt(True, max_disparity=DR.ZUPT_TEST_MAX_DISPARITY)
    off.set_zupt(False)                                                # switched on and off again before the first frame
    Hv, Rz = _selector(6), 0.05 * 0.05 * np.eye(3)
    fired, first = [], None
    vn = {"on": [], "off": []}
    for k in range(RUN_FRAMES):
        before = on.num_zupt()
        on.run(k, 1, threaded=False)
        off.run(k, 1, threaded=False)
        s_on, s_off = on.imu_state(), off.imu_state()
        if on.num_zupt() > before:
            fired.append(k)
        if 21 <= k <= 60:
            vn["on"].append(np.linalg.norm(s_on[7:10]))
            vn["off"].append(np.linalg.norm(s_off[7:10]))
        if first is None and fired:
            # the first zero-velocity frame: the off-run's state and covariance + the restatement's update
            first = k
            want = DR.direct_update_fixed(off.cov(), Hv, 0.0 - s_off[7:10], Rz, gate=CHI2_95_DOF3)
            assert want["status"] == 1
            assert np.array_equal(on.cov(), want["P"])
            p, v = _state_plus(s_off, want["dx"])
            assert np.array_equal(s_on[4:7], p) and np.array_equal(s_on[7:10], v)
            assert np.abs(on.poses()["p"][-1] - s_on[4:7]).max() < 1e-12
        elif first is None:
            assert np.array_equal(s_on, s_off) and np.array_equal(on.cov(), off.cov())
        elif k <= 60:
            assert np.trace(on.cov()[6:9, 6:9]) < np.trace(off.cov()[6:9, 6:9]), k
        if k == 59:
            p_end = (np.linalg.norm(s_on[4:7]), np.linalg.norm(s_off[4:7]))
    print("zero-velocity updates at frames %d..%d (%d); mean |v| over frames 21..60: on %.3e m/s, off %.3e m/s; |p| at frame 59: on %.3e m, off %.3e m"
          % (fired[0], fired[-1], len(fired), np.mean(vn["on"]), np.mean(vn["off"]), p_end[0], p_end[1]))
    assert set(range(21, 61)) <= set(fired) and not [k for k in fired if k >= 66]
    assert on.num_direct_updates() == on.num_zupt() == len(fired)
    assert np.mean(vn["on"]) <= np.mean(vn["off"])
    assert on.num_resets() == 0 and off.num_resets() == 0
    # pipelined == lockstep, bitwise, with the update on
    piped.run(0, RUN_FRAMES, pipelined=True)
    assert piped.num_zupt() == on.num_zupt()
    assert np.array_equal(piped.poses(), on.poses()) and np.array_equal(piped.cov(), on.cov()) and np.array_equal(piped.imu_state(), on.imu_state())
    # off == a Runner that never heard of it
    plain.run(0, RUN_FRAMES, threaded=False)
    assert np.array_equal(off.poses(), plain.poses()) and np.array_equal(off.cov(), plain.cov())
    assert np.array_equal(off.dump()[0], plain.dump()[0]) and off.num_updates() == plain.num_updates()
    assert off.num_direct_updates() == off.num_zupt() == 0 and not np.array_equal(on.poses(), off.poses())
    for r in (on, off, plain, piped):
        r.close()


# ------------------------------------------------------------------------------------------------ 7. app
def test_app_zupt_keys(tmp_path, oracle):
    """run_euroc_single_thread with `zupt: on` in app_msckfvio.yaml writes the pose file of a Runner with set_zupt(True) fed the
    same files, line by line; without the keys the pose file of a plain Runner."""
    from PIL import Image
    from msckf_stereo_c_amd import build
    build.build_all()
    n_frames = 30
    syn = oracle.Synth(seed=0x5EED0042, width=752, height=480, n_static=26, motion_scale=3.0)
    mav0 = tmp_path / "mav0"
    for c in (0, 1):
        (mav0 / ("cam%d" % c) / "data").mkdir(parents=True)
    (mav0 / "imu0").mkdir()
    rows, images = [], []
    for k in range(n_frames):
        a, b = syn.render(k)
        images.append((a, b))
        name = "%d.png" % (T0_NS + k * DT_NS)
        Image.fromarray(a).save(mav0 / "cam0" / "data" / name, compress_level=1)
        Image.fromarray(b).save(mav0 / "cam1" / "data" / name, compress_level=1)
        rows.append("%d,%s\r" % (T0_NS + k * DT_NS, name))
    for c in (0, 1):
        (mav0 / ("cam%d" % c) / "data.csv").write_text("#timestamp [ns],filename\r\n" + "\n".join(rows) + "\n")
    lines, samples = ["#timestamp [ns],w_x,w_y,w_z,a_x,a_y,a_z"], []
    for j in range((n_frames + 2) * 10):
        s = syn.imu(j)
        text = ["%.9g" % v for v in list(s.angular_velocity) + list(s.linear_acceleration)]
        ns = T0_NS + j * (DT_NS // 10)
        lines.append("%d,%s" % (ns, ",".join(text)))
        m = ImuSample()                                   # what the app makes of the line: stamp as below, values through a float
        m.time_stamp = (float(ns // 1000000000) * 1e9 + float(ns % 1000000000)) * 1e-9
        vals = [float(np.float32(x)) for x in text]
        m.angular_velocity[:], m.linear_acceleration[:] = vals[:3], vals[3:]
        samples.append(m)
    (mav0 / "imu0" / "data.csv").write_text("\n".join(lines) + "\n")
    exe = os.path.join(ROOT, "msckf_stereo_c_amd", "_build", "run_euroc_single_thread")
    stock = open(os.path.join(ROOT, "config", "app_msckfvio.yaml")).read()
    host = C.CDLL(os.path.join(ROOT, "msckf_stereo_c_amd", "_build", "libmskf_host.so"))
    calib, fe, ekf = Calib(), FeCfg(), EkfCfg()
    assert host.mskfh_load_configs(os.path.join(ROOT, "config").encode(), C.byref(calib), C.byref(fe), C.byref(ekf)) == 0

    def app_lines(keys):
        top = tmp_path / ("run_%d" % len(keys))
        (top / "config").mkdir(parents=True)
        for f in ("camchain-imucam-euroc.yaml", "app_imgproc.yaml"):
            (top / "config" / f).write_text(open(os.path.join(ROOT, "config", f)).read())
        (top / "config" / "app_msckfvio.yaml").write_text(stock + "\n" + keys)
        (top / "build").mkdir()
        res = subprocess.run([exe, str(mav0)], cwd=top / "build", capture_output=True, text=True, timeout=300)
        assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
        return (top / "build" / "pose_out.txt").read_text().splitlines()

    def runner_lines(zupt):
        run = RN.Runner(calib, fe, ekf)
        if zupt:
            run.set_zupt(True)
        j = 0
        for k in range(n_frames):
            t_img = _frame_time(k)
            while True:
                m = samples[j]
                j += 1
                run.imu(0, m)
                if not (m.time_stamp <= t_img):
                    break
            run.step([images[k][0]], [images[k][1]], [t_img])
        out = ["%.6f %.6f %.6f %.6f %.6f %.6f %.6f %.6f" % ((r["t"],) + tuple(r["p"]) + tuple(r["q"])) for r in run.poses()]
        n_zupt = run.num_zupt()
        run.close()
        return out, n_zupt
    plain, n0 = runner_lines(False)
    with_zupt, n1 = runner_lines(True)
    assert n0 == 0 and n1 >= 3 and len(plain) == len(with_zupt) > 5 and plain != with_zupt
    assert app_lines("") == plain
    assert app_lines("zupt: on\n") == with_zupt
