"""GPU tests of the prediction half of the filter and of the staging copies, entry point by entry point:

  * k_ekf_propagate building Phi and Q itself from mskf_imu_step records (mskf_ekf_propagate_imu, mskf_ekf_predict_batch,
    the fused augmentation), against the long-double restatement of processModel / stateAugmentation in ekf_reference.py;
  * k_ekf_remove_clone with one or two clones per stream (mskf_ekf_remove_clones_batch), against numpy deletion;
  * every source of the position variances onlineReset reads, against diag(P);
  * k_mskf_copy (fe_launch_copy), byte for byte.

Bars: Phi max |dPhi| <= 1e-14, Q max |dQ| / max |Q| <= 1e-13, P per block (P_II, P_IC, new clone rows) max |dP| / max |P|
<= 1e-12; exact symmetry and untouched blocks bit for bit.  test_ekf_reference.py shows that a wrong series term, fix-up,
Phi(0,0), F block or noise density moves these quantities 1e4 times beyond the bars.
"""
import ctypes as C

import numpy as np
import pytest

from msckf_stereo_c_amd import capi
from msckf_stereo_c_amd.ctypes_types import default_ekf_cfg, default_fe_cfg

import ekf_problems
import ekf_reference as R
from hip_runtime import Hip as _Hip

pytestmark = pytest.mark.gpu

LD = R.LD
N = 21
ERR_INVALID, ERR_CAPACITY = -1, -4
GYRO = {"zero": (0.0, 0.0, 0.0), "fast": (0.0, 3.0, 0.0)}         # |w| = 3 rad/s
ATT = {"near_identity": R.quat_axis_angle((1.0, -2.0, 0.5), 1e-3), "near_180": R.quat_axis_angle((0.3, -1.0, 0.5), np.pi - 1e-3),
       "general": R.quat_axis_angle((1.0, 2.0, 3.0), 2.0)}


def _stream(gpu_ctx, oracle, max_clones, **kw):
    calib = oracle.euroc_calib(376, 240)
    cfg = default_ekf_cfg(max_cam_state_size=max_clones, **kw)
    return capi.Stream(gpu_ctx, calib, default_fe_cfg(), cfg)


def _qc():
    return R.qc_of(default_ekf_cfg())


def _rel(got, ref):
    ref = np.asarray(ref, dtype=LD)
    return float(np.abs(np.asarray(got, dtype=LD) - ref).max() / max(np.abs(ref).max(), LD(1e-300)))


def _predict_ref(P0, steps, J):
    P = R.propagate(P0, steps, _qc())[0] if len(steps) else np.asarray(P0, dtype=LD)
    return R.augment(P, J) if J is not None else P


def _check_predicted(got, P0, steps, J, tag=""):
    """got (device, after propagation over `steps` and augmentation with J) against the reference; returns the errors."""
    d = P0.shape[0]
    ref = _predict_ref(P0, steps, J)
    assert got.shape == ref.shape, tag
    assert np.array_equal(got, got.T), tag
    assert np.array_equal(got[N:d, N:d], P0[N:, N:]), tag               # P_CC is not touched
    err = R.block_errors(got[:, :d] if J is not None else got, ref[:, :d] if J is not None else ref)
    if J is not None:
        err["new"] = _rel(got[d:, :], ref[d:, :])
    for k, e in err.items():
        assert e <= 1e-12, (tag, k, e)
    return err


# ------------------------------------------------------------------------------------------------ a. Phi and Q, read back
@pytest.mark.parametrize("att", ["near_identity", "near_180"])
@pytest.mark.parametrize("gyro", ["zero", "fast"])
@pytest.mark.parametrize("dt", [0.0, 0.005, 0.02])
def test_device_phi_and_q_read_back(gpu_ctx, oracle, dt, gyro, att):
    """P = [[0, I 0], [I 0, 0]] with 4 clones (d = 45): one mskf_ekf_propagate_imu call over k steps leaves the device's
    Phi_k ... Phi_1 in P_IC[:, :21] and its accumulated noise in P_II (for k = 1 exactly sym(Q)).  Element by element
    against the long-double reference: |dPhi| <= 1e-14, |dQ| / max |Q| <= 1e-13, and the device's own Phi satisfies the
    observability constraints to 1e-13.  Observed on MI355X: |dPhi| <= 4.7e-15 (40 steps of 20 ms near 180 deg),
    |dQ| / |Q| <= 1.7e-15, constraint residual <= 6.9e-17 (relative to max(1, |w|)); dt = 0 gives Q = 0 exactly."""
    s = _stream(gpu_ctx, oracle, 4)
    d = N + 6 * 4
    P0 = np.zeros((d, d))
    P0[:N, N:2 * N] = np.eye(N)
    P0[N:2 * N, :N] = np.eye(N)
    worst = [0.0, 0.0, 0.0]
    for n_steps in (1, 2, 10, 40):
        steps = R.imu_steps(n_steps, dt, gyro=GYRO[gyro], q0=ATT[att])
        s.ekf_set_cov(P0)
        s.ekf_propagate_imu(steps)
        P = s.ekf_get_cov()
        Pref, Phis, Qs = R.propagate(P0, steps, _qc())
        Phi_dev, Q_dev = P[:N, N:2 * N], P[:N, :N]
        e_phi = float(np.abs(Phi_dev - R.compose(Phis)).max())
        assert e_phi <= 1e-14, (n_steps, e_phi)
        assert np.array_equal(P[N:2 * N, :N], Phi_dev.T)
        assert not P[:N, 2 * N:].any() and not P[N:, N:].any()           # the other clones' cross terms stay 0, P_CC too
        if dt == 0.0:
            assert not Q_dev.any()
            e_q = 0.0
        else:
            e_q = _rel(Q_dev, Pref[:N, :N])
            assert e_q <= 1e-13, (n_steps, e_q)
        assert np.array_equal(Q_dev, Q_dev.T)
        if n_steps == 1:
            st = steps[0]
            u = np.asarray(st["u"], dtype=LD)
            for rows, w in ((slice(6, 9), st["w1"]), (slice(12, 15), st["w2"])):
                w = np.asarray(w, dtype=LD)
                res = float(np.abs(np.asarray(Phi_dev[rows, 0:3], dtype=LD) @ u - w).max()) / max(1.0, float(np.abs(w).max()))
                assert res <= 1e-13, (rows, res)
                worst[2] = max(worst[2], res)
        worst[0], worst[1] = max(worst[0], e_phi), max(worst[1], e_q)
    print("dt %g gyro %s att %s: |dPhi| %.1e  |dQ|/|Q| %.1e  constraint %.1e" % (dt, gyro, att, *worst))
    s.close()


# ------------------------------------------------------------------------------------------------ b. realistic P
@pytest.mark.parametrize("n_clones,max_clones", [(0, 4), (1, 4), (39, 39), (40, 40), (64, 64), (1, 30)])
def test_propagate_imu_realistic_covariance(gpu_ctx, oracle, n_clones, max_clones):
    """mskf_ekf_propagate_imu on an SPD covariance: d = 21, 27, 255 / 261 (either side of the kernel's 256-column sweep),
    405 (64 clones, ld = 408 != d) and a window with room for more clones than it holds (d = 27, ld = 208).  Per block
    against the stepwise long-double reference (the device applies the composed transition to P_IC once), P_CC bit for
    bit, exact symmetry.  Observed on MI355X: P_II <= 9.5e-16 (d = 405), P_IC <= 3.0e-16."""
    d = N + 6 * n_clones
    rng = np.random.default_rng(1000 + d)
    s = _stream(gpu_ctx, oracle, max_clones)
    P0 = R.spd(d, rng)
    s.ekf_set_cov(P0)
    steps = R.imu_steps(12, 0.005, gyro=GYRO["fast"], q0=ATT["general"], seed=d, jitter=0.05)
    s.ekf_propagate_imu(steps[:5])
    s.ekf_propagate_imu(steps[5:])                                     # two calls: the first result is the second's input
    err = _check_predicted(s.ekf_get_cov(), P0, steps, None, "d=%d" % d)
    print("d %d ld-room %d: %s" % (d, max_clones, {k: "%.1e" % v for k, v in err.items()}))
    s.close()


# ------------------------------------------------------------------------------------------------ c. predict batch
BATCH = [   # (clones, max clones, IMU steps, augment)
    (1, 8, 0, True),       # augmentation only
    (39, 40, 7, False),    # propagation only, d = 255
    (40, 45, 12, True),    # both, d = 261 -> 267
    (4, 6, 0, False),      # neither: P stays bit-identical
    (0, 4, 3, True),       # both, d = 21 -> 27
    (63, 64, 5, True),     # both, to the 64-clone maximum d = 405
]


def _batch_inputs():
    rng = np.random.default_rng(77)
    out = []
    for i, (nc, mc, ns, aug) in enumerate(BATCH):
        d = N + 6 * nc
        steps = R.imu_steps(ns, 0.005, gyro=(0.3 * i, -2.0, 1.0), q0=ATT["general" if i % 2 else "near_180"], seed=i, jitter=0.05)
        out.append((R.spd(d, rng), steps, R.augment_jacobian(rng) if aug else None))
    return out


def test_predict_batch(gpu_ctx, oracle):
    """mskf_ekf_predict_batch over six streams of different sizes (augmentation only, propagation only, both, neither):
    each stream matches the reference at the bars of the realistic-P test, the same stream alone in a batch of one bit for
    bit, and mskf_ekf_propagate_imu followed by mskf_ekf_augment bit for bit (the header calls them equivalent; they form
    the same sums in the same order).  Observed on MI355X: P_II <= 9.3e-16, P_IC <= 2.5e-16, new clone rows <= 3.6e-16.
    Then the three single-stream calls on a fresh context, each staging more bytes than every call before it there (the
    context's staging arena grows between them), against the reference at the same bars."""
    inputs = _batch_inputs()

    def fresh():
        ss = [_stream(gpu_ctx, oracle, mc) for (_, mc, _, _) in BATCH]
        for s, (P0, _, _) in zip(ss, inputs):
            s.ekf_set_cov(P0)
        return ss

    ss = fresh()
    gpu_ctx.ekf_predict_batch(ss, [x[1] for x in inputs], [x[2] for x in inputs])
    together = [s.ekf_get_cov() for s in ss]
    for s in ss:
        s.close()
    ss = fresh()
    alone = []
    for s, (_, steps, J) in zip(ss, inputs):
        gpu_ctx.ekf_predict_batch([s], [steps], [J])
        alone.append(s.ekf_get_cov())
    for s in ss:
        s.close()
    ss = fresh()
    separate = []
    for s, (_, steps, J) in zip(ss, inputs):
        if len(steps):
            s.ekf_propagate_imu(steps)
        if J is not None:
            s.ekf_augment(J)
        separate.append(s.ekf_get_cov())
    for s in ss:
        s.close()
    for i, ((P0, steps, J), P) in enumerate(zip(inputs, together)):
        assert np.array_equal(P, alone[i]), i
        assert np.array_equal(P, separate[i]), i
        if not len(steps) and J is None:
            assert np.array_equal(P, P0)
            continue
        err = _check_predicted(P, P0, steps, J, "stream %d" % i)
        print("stream %d d %d steps %d J %s: %s" % (i, P0.shape[0], len(steps), J is not None, {k: "%.1e" % v for k, v in err.items()}))
    ctx = capi.Context(0)
    try:
        rng = np.random.default_rng(78)
        s = _stream(ctx, oracle, 40)
        P0 = R.spd(N + 6 * 30, rng)
        s.ekf_set_cov(P0)
        J = R.augment_jacobian(rng)
        steps = R.imu_steps(40, 0.005, gyro=GYRO["fast"], q0=ATT["general"], seed=78, jitter=0.05)
        s.ekf_augment(J)                                                   # descriptor + J: 640 bytes
        P1 = s.ekf_get_cov()
        _check_predicted(P1, P0, [], J, "fresh context, augment")
        s.ekf_propagate_imu(steps)                                         # + 40 IMU steps: 12 KiB
        P2 = s.ekf_get_cov()
        _check_predicted(P2, P1, steps, None, "fresh context, propagate_imu")
        _, Phis, Qs = R.propagate(P2, steps[:4], _qc())
        s.ekf_propagate(np.array(Phis, dtype=np.float64), np.array(Qs, dtype=np.float64))     # + 4 (Phi, Q) pairs: 28 KiB
        _check_predicted(s.ekf_get_cov(), P2, steps[:4], None, "fresh context, propagate")
        s.close()
    finally:
        ctx.close()


def test_predict_batch_capacity_changes_nothing(gpu_ctx, oracle):
    """A stream already at its clone capacity asked to augment: MSKF_ERR_CAPACITY, and no stream of the batch changes."""
    rng = np.random.default_rng(5)
    ss = [_stream(gpu_ctx, oracle, 8), _stream(gpu_ctx, oracle, 4), _stream(gpu_ctx, oracle, 8)]
    Ps = [R.spd(N + 6 * 3, rng), R.spd(N + 6 * 4, rng), R.spd(N + 6 * 2, rng)]
    for s, P in zip(ss, Ps):
        s.ekf_set_cov(P)
    steps = R.imu_steps(4, 0.005, gyro=GYRO["fast"], q0=ATT["general"])
    J = R.augment_jacobian(rng)
    with pytest.raises(capi.MskfError) as e:
        gpu_ctx.ekf_predict_batch(ss, [steps, steps, steps], [J, J, J])
    assert e.value.code == ERR_CAPACITY
    for s, P in zip(ss, Ps):
        assert s.ekf_dim() == P.shape[0]
        assert np.array_equal(s.ekf_get_cov(), P)
    with pytest.raises(capi.MskfError) as e:
        ss[1].ekf_augment(J)
    assert e.value.code == ERR_CAPACITY and np.array_equal(ss[1].ekf_get_cov(), Ps[1])
    for s in ss:
        s.close()


# ------------------------------------------------------------------------------------------------ d. clone removal
def _delete(P, pair):
    drop = set()
    for c in pair:
        if c >= 0:
            drop |= set(range(N + 6 * c, N + 6 * c + 6))
    keep = [i for i in range(P.shape[0]) if i not in drop]
    return P[np.ix_(keep, keep)]


REMOVALS = [   # (clones, pair)
    (8, (2, 5)), (8, (5, 2)), (8, (3, -1)), (8, (-1, 4)), (8, (0, 7)), (8, (3, 4)), (8, (7, 6)), (8, (-1, -1)), (20, (0, 19)),
    (5, (4, -1)), (5, (0, 1)),
]


def test_remove_clones_batch(gpu_ctx, oracle):
    """mskf_ekf_remove_clones_batch (pruneCamStateBuffer's two clones per stream): pairs in either order, (a, -1) and
    (-1, a), first and last clone, adjacent and apart, (-1, -1) streams in the same batch; bit for bit against numpy
    deletion.  Each stream is then predicted and updated, and a second removal follows: the update result equals that of a
    fresh stream given the same covariance bit for bit, so a stale P / P_alt pointer or ld after the swap would show."""
    calib = oracle.euroc_calib(376, 240)
    rng = np.random.default_rng(9)
    ss = [_stream(gpu_ctx, oracle, 20) for _ in REMOVALS]
    Ps = [R.spd(N + 6 * nc, rng) for nc, _ in REMOVALS]
    for s, P in zip(ss, Ps):
        s.ekf_set_cov(P)
    gpu_ctx.ekf_remove_clones_batch(ss, [p for _, p in REMOVALS])
    Ps = [_delete(P, p) for P, (_, p) in zip(Ps, REMOVALS)]
    for i, (s, P) in enumerate(zip(ss, Ps)):
        assert s.ekf_dim() == P.shape[0], i
        assert np.array_equal(s.ekf_get_cov(), P), i
    # predict on the swapped buffers
    steps = [R.imu_steps(4, 0.005, gyro=GYRO["fast"], q0=ATT["general"], seed=i, jitter=0.05) for i in range(len(ss))]
    Js = [R.augment_jacobian(rng) for _ in ss]
    gpu_ctx.ekf_predict_batch(ss, steps, Js)
    for i, s in enumerate(ss):
        Pn = s.ekf_get_cov()
        _check_predicted(Pn, Ps[i], steps[i], Js[i], "removal %d" % i)
        Ps[i] = Pn
    # update on the swapped buffers == the same update on a stream that never removed a clone
    for i, s in enumerate(ss):
        nc = (Ps[i].shape[0] - N) // 6
        pr = ekf_problems.make_problem(calib, seed=500 + i, n_clones=nc, n_feat=6, min_obs=min(3, nc))
        kw = dict(gravity=pr["gravity"], clones=pr["clones"], positions=pr["positions"], obs_start=pr["obs_start"],
                  obs_clone=pr["obs_clone"], obs_z=pr["obs_z"], dof_offset=-1, apply_row_cap=True)
        got = s.ekf_update(**kw)
        f = _stream(gpu_ctx, oracle, 20)
        f.ekf_set_cov(Ps[i])
        want = f.ekf_update(**kw)
        assert got["rows"] == want["rows"] > 0, i
        assert np.array_equal(got["delta_x"], want["delta_x"]), i
        Ps[i] = s.ekf_get_cov()
        assert np.array_equal(Ps[i], f.ekf_get_cov()), i
        assert np.array_equal(got["pos_var"], np.diag(Ps[i])[12:15]), i
        f.close()
    # second removal: back onto the first buffer
    pairs = [(0, -1)] * len(ss)
    gpu_ctx.ekf_remove_clones_batch(ss, pairs)
    for i, s in enumerate(ss):
        want = _delete(Ps[i], (0, -1))
        assert s.ekf_dim() == want.shape[0] and np.array_equal(s.ekf_get_cov(), want), i
    for s in ss:
        s.close()


def test_remove_clones_batch_refuses_bad_indices(gpu_ctx, oracle):
    """a == b, an index at or beyond the clone count (in either slot), also behind a valid stream in the same batch:
    MSKF_ERR_INVALID and no covariance or dimension changes."""
    rng = np.random.default_rng(12)
    ss = [_stream(gpu_ctx, oracle, 8), _stream(gpu_ctx, oracle, 8)]
    Ps = [R.spd(N + 6 * 5, rng), R.spd(N + 6 * 3, rng)]
    for s, P in zip(ss, Ps):
        s.ekf_set_cov(P)
    for bad in ((2, 2), (3, -1), (-1, 3), (0, 3), (7, 1)):
        with pytest.raises(capi.MskfError) as e:
            gpu_ctx.ekf_remove_clones_batch(ss, [(1, 4), bad])
        assert e.value.code == ERR_INVALID, bad
        for s, P in zip(ss, Ps):
            assert s.ekf_dim() == P.shape[0] and np.array_equal(s.ekf_get_cov(), P), bad
    with pytest.raises(capi.MskfError) as e:
        ss[1].ekf_remove_clone(3)
    assert e.value.code == ERR_INVALID and np.array_equal(ss[1].ekf_get_cov(), Ps[1])
    for s in ss:
        s.close()


# ------------------------------------------------------------------------------------------------ e. position variances
def _pv(P):
    return np.diag(P)[12:15].copy()


def _all_pos_var_reads(gpu_ctx, ss):
    """Every read-out entry point, each against diag(P)[12:15] of mskf_ekf_get_cov, bit for bit."""
    want = [_pv(s.ekf_get_cov()) for s in ss]
    for s, w in zip(ss, want):
        assert np.array_equal(s.ekf_pos_var(), w)
    assert np.array_equal(gpu_ctx.ekf_pos_var_batch(ss), np.array(want))
    out = gpu_ctx.ekf_pos_var_batch_begin(ss)
    gpu_ctx.ekf_pos_var_batch_end()
    assert np.array_equal(out, np.array(want))


def test_pos_var_read_outs(gpu_ctx, oracle):
    """mskf_ekf_get_pos_var, _batch and _begin / _end after a predict, an update and a clone removal."""
    calib = oracle.euroc_calib(376, 240)
    rng = np.random.default_rng(21)
    ss = [_stream(gpu_ctx, oracle, 12), _stream(gpu_ctx, oracle, 40)]
    for s, nc in zip(ss, (6, 39)):
        s.ekf_set_cov(R.spd(N + 6 * nc, rng))
    gpu_ctx.ekf_predict_batch(ss, [R.imu_steps(6, 0.005, gyro=GYRO["fast"], q0=ATT["general"])] * 2, [R.augment_jacobian(rng), None])
    _all_pos_var_reads(gpu_ctx, ss)
    pr = ekf_problems.make_problem(calib, seed=3, n_clones=7, n_feat=10)
    got = ss[0].ekf_update(pr["gravity"], pr["clones"], pr["positions"], pr["obs_start"], pr["obs_clone"], pr["obs_z"], -1, True)
    assert got["rows"] > 0 and np.array_equal(got["pos_var"], _pv(ss[0].ekf_get_cov()))
    _all_pos_var_reads(gpu_ctx, ss)
    gpu_ctx.ekf_remove_clones_batch(ss, [(0, 6), (-1, 20)])
    _all_pos_var_reads(gpu_ctx, ss)
    for s in ss:
        s.close()


def _outliers(pr):
    """Every observation pushed 0.3 (normalised) off, alternately: every feature fails the gate."""
    pr = dict(pr)
    z = pr["obs_z"].copy()
    z += 0.3 * np.where(np.arange(len(z)) % 2 == 0, 1.0, -1.0)[:, None]
    pr["obs_z"] = z
    return pr


UPDATE_ROUTES = [   # (name, compression mode, make_problem kwargs, dof_offset, row cap, expected used_qr or None)
    ("gram", 1, dict(n_clones=20, n_feat=30, seed=2), -1, True, 0),
    ("tsqr", 2, dict(n_clones=20, n_feat=30, seed=2), -1, True, 1),
    ("uncompressed", 0, dict(n_clones=13, n_feat=2, seed=1301, min_obs=3), -1, True, 2),
    ("pairs", 3, dict(n_clones=12, n_feat=70, seed=32, pair=(0, 1)), 0, False, None),
    ("small", 0, dict(n_clones=4, n_feat=12, seed=8, min_obs=3), -1, True, None),      # 24 active columns, not pairs
    ("gated_out", 0, dict(n_clones=10, n_feat=8, seed=4, min_obs=3), -1, True, None),
]


@pytest.mark.parametrize("name,mode,kw,dof,cap,used", UPDATE_ROUTES, ids=[r[0] for r in UPDATE_ROUTES])
def test_pos_var_out_of_update(gpu_ctx, oracle, name, mode, kw, dof, cap, used):
    """mskf_ekf_update_args.pos_var_out equals diag(P)[12:15] after the update bit for bit on every route: the epilogue of
    k_ekf_gemm<PUPD> after Gram + Cholesky, Householder TSQR, the uncompressed stack, the pair kernels + fused small update,
    the fused small update alone, and a stream whose every feature fails the gate (rows == 0: P must not change)."""
    calib = oracle.euroc_calib(376, 240)
    s = _stream(gpu_ctx, oracle, max(kw["n_clones"], 4), compression_mode=mode)
    pr = ekf_problems.make_problem(calib, **kw)
    if name == "gated_out":
        pr = _outliers(pr)
    s.ekf_set_cov(pr["P"])
    got = s.ekf_update(pr["gravity"], pr["clones"], pr["positions"], pr["obs_start"], pr["obs_clone"], pr["obs_z"], dof, cap)
    P = s.ekf_get_cov()
    if name == "gated_out":
        assert got["rows"] == 0 and np.array_equal(P, pr["P"])
    else:
        assert got["rows"] > 0
    if used is not None:
        assert got["used_qr"] == used
    assert np.array_equal(got["pos_var"], _pv(P)), (got["pos_var"], _pv(P))
    s.close()


def test_pos_var_out_of_batches(gpu_ctx, oracle):
    """Streams without features in a batch where others update get their variances from k_ekf_posvar_upd; a batch in which
    no stream has features launches nothing and reports -1."""
    calib = oracle.euroc_calib(376, 240)
    rng = np.random.default_rng(31)
    pr = ekf_problems.make_problem(calib, seed=6, n_clones=10, n_feat=12)
    ss = [_stream(gpu_ctx, oracle, 12) for _ in range(3)]
    ss[0].ekf_set_cov(R.spd(N + 6 * 3, rng))
    ss[1].ekf_set_cov(pr["P"])
    ss[2].ekf_set_cov(R.spd(N + 6 * 12, rng))

    def empty(nc):
        return dict(gravity=pr["gravity"], clones=np.zeros((nc, 14)), positions=None, obs_start=[0], obs_clone=np.zeros(0, np.int32),
                    obs_z=np.zeros((0, 4)), dof_offset=-1, apply_row_cap=True)
    full = dict(gravity=pr["gravity"], clones=pr["clones"], positions=pr["positions"], obs_start=pr["obs_start"], obs_clone=pr["obs_clone"],
                obs_z=pr["obs_z"], dof_offset=-1, apply_row_cap=True)
    res = gpu_ctx.ekf_update_batch(ss, [empty(3), full, empty(12)])
    assert res[1]["rows"] > 0 and res[0]["rows"] == res[2]["rows"] == 0
    for s, r in zip(ss, res):
        assert np.array_equal(r["pos_var"], _pv(s.ekf_get_cov()))
    res = gpu_ctx.ekf_update_batch([ss[0], ss[2]], [empty(3), empty(12)])
    for r in res:
        assert np.array_equal(r["pos_var"], np.full(3, -1.0))
    res = ss[0].ekf_update(**empty(3))
    assert np.array_equal(res["pos_var"], np.full(3, -1.0))
    for s in ss:
        s.close()


def test_pending_pos_var_read_out_blocks_predict_and_removal(gpu_ctx, oracle):
    """While a mskf_ekf_get_pos_var_batch_begin is pending (its kernel reads descriptors from the arena they would reuse),
    mskf_ekf_predict_batch, mskf_ekf_remove_clones_batch and the single-stream mskf_ekf_propagate, mskf_ekf_propagate_imu and
    mskf_ekf_augment refuse and change nothing; after _end all of them work again."""
    rng = np.random.default_rng(41)
    s = _stream(gpu_ctx, oracle, 8)
    P0 = R.spd(N + 6 * 4, rng)
    s.ekf_set_cov(P0)
    steps = R.imu_steps(3, 0.005, gyro=GYRO["fast"], q0=ATT["general"])
    J = R.augment_jacobian(rng)
    Phis, Qs = (np.array(x, dtype=np.float64) for x in R.propagate(P0, steps, _qc())[1:])
    out = gpu_ctx.ekf_pos_var_batch_begin([s])
    try:
        with pytest.raises(capi.MskfError) as e:
            gpu_ctx.ekf_predict_batch([s], [steps], [J])
        assert e.value.code == ERR_INVALID
        with pytest.raises(capi.MskfError) as e:
            gpu_ctx.ekf_remove_clones_batch([s], [(0, 1)])
        assert e.value.code == ERR_INVALID
        with pytest.raises(capi.MskfError) as e:
            s.ekf_propagate(Phis, Qs)
        assert e.value.code == ERR_INVALID
        with pytest.raises(capi.MskfError) as e:
            s.ekf_propagate_imu(steps)
        assert e.value.code == ERR_INVALID
        with pytest.raises(capi.MskfError) as e:
            s.ekf_augment(J)
        assert e.value.code == ERR_INVALID
    finally:
        gpu_ctx.ekf_pos_var_batch_end()
    assert np.array_equal(out[0], _pv(P0))
    assert s.ekf_dim() == P0.shape[0] and np.array_equal(s.ekf_get_cov(), P0)
    gpu_ctx.ekf_predict_batch([s], [steps], [J])
    _check_predicted(s.ekf_get_cov(), P0, steps, J)
    gpu_ctx.ekf_remove_clones_batch([s], [(0, 1)])
    assert s.ekf_dim() == P0.shape[0] + 6 - 12
    P1 = s.ekf_get_cov()
    s.ekf_propagate(Phis, Qs)
    P2 = s.ekf_get_cov()
    _check_predicted(P2, P1, steps, None)
    s.ekf_propagate_imu(steps)
    P3 = s.ekf_get_cov()
    _check_predicted(P3, P2, steps, None)
    s.ekf_augment(J)
    _check_predicted(s.ekf_get_cov(), P3, [], J)
    s.close()


def _work_beside_a_pending_read_out(parent, child, oracle):
    """A position-variance read-out pending on `parent` (which then refuses predictions) while `child` runs a prediction batch
    and an update batch to completion, each on a stream of its own.  Returns (read-out, P after prediction, P after update,
    update rows) and the inputs."""
    rng = np.random.default_rng(47)
    calib = oracle.euroc_calib(376, 240)
    pr = ekf_problems.make_problem(calib, seed=6, n_clones=10, n_feat=12)
    P0, P1 = R.spd(N + 6 * 4, rng), R.spd(N + 6 * 5, rng)
    J = R.augment_jacobian(rng)
    steps = R.imu_steps(6, 0.005, gyro=GYRO["fast"], q0=ATT["general"], seed=47, jitter=0.05)
    p, a, b = _stream(parent, oracle, 8), _stream(child, oracle, 8), _stream(child, oracle, 12)
    p.ekf_set_cov(P0)
    a.ekf_set_cov(P1)
    b.ekf_set_cov(pr["P"])
    full = dict(gravity=pr["gravity"], clones=pr["clones"], positions=pr["positions"], obs_start=pr["obs_start"], obs_clone=pr["obs_clone"],
                obs_z=pr["obs_z"], dof_offset=-1, apply_row_cap=True)
    out = parent.ekf_pos_var_batch_begin([p])
    try:
        with pytest.raises(capi.MskfError) as e:
            parent.ekf_predict_batch([p], [steps], [J])
        assert e.value.code == ERR_INVALID
        child.ekf_predict_batch([a], [steps], [J])
        res = child.ekf_update_batch([b], [full])
    finally:
        parent.ekf_pos_var_batch_end()
    got = (out[0].copy(), a.ekf_get_cov(), b.ekf_get_cov(), res[0]["rows"])
    for s in (p, a, b):
        s.close()
    return got, (P0, P1, pr["P"], steps, J)


def test_shared_context_beside_a_pending_batch_of_its_parent(gpu_ctx, oracle):
    """mskf_ctx_create_shared: a second context with staging arenas of its own that enqueues on its parent's HIP stream.  It
    reports the parent's stream; while a read-out is pending on the parent, a prediction batch and an update batch run to
    completion on the shared context (their arenas are not the pending batch's); the covariances are bit-identical to the
    same work on two independent contexts; and destroying the shared context first leaves the parent usable."""
    shared = capi.Context(shared_with=gpu_ctx)
    try:
        assert shared.hip_stream() == gpu_ctx.hip_stream()
        (pv, Pa, Pb, rows), (P0, P1, Pu, steps, J) = _work_beside_a_pending_read_out(gpu_ctx, shared, oracle)
    finally:
        shared.close()
    c1, c2 = capi.Context(0), capi.Context(0)
    try:
        assert c1.hip_stream() != c2.hip_stream()
        (pv_i, Pa_i, Pb_i, rows_i), _ = _work_beside_a_pending_read_out(c1, c2, oracle)
    finally:
        c2.close()
        c1.close()
    assert np.array_equal(pv, _pv(P0)) and np.array_equal(pv_i, pv)
    _check_predicted(Pa, P1, steps, J)
    assert rows > 0 and not np.array_equal(Pb, Pu)
    assert np.array_equal(Pa, Pa_i) and np.array_equal(Pb, Pb_i) and rows == rows_i
    # the parent, its shared context destroyed
    s = _stream(gpu_ctx, oracle, 8)
    s.ekf_set_cov(P0)
    gpu_ctx.ekf_predict_batch([s], [steps], [J])
    P2 = s.ekf_get_cov()
    _check_predicted(P2, P0, steps, J)
    assert np.array_equal(gpu_ctx.ekf_pos_var_batch([s])[0], _pv(P2))
    s.close()


# ------------------------------------------------------------------------------------------------ f. staging copies
CANARY = 64      # bytes after each destination that must survive the copy
MiB = 1 << 20
COPY_CASES = [   # segments of one launch: (bytes, direction)
    [(1, "h2d")],
    [(15, "d2h"), (16, "d2d"), (17, "h2d")],
    [(4095, "d2d"), (1, "d2h"), (17, "d2d"), (15, "h2d"), (16, "d2h"), (4095, "h2d")],   # six segments, odd tails
    [(4 * 16384, "h2d")],                       # 4 workgroups, one trip of the 4-deep unrolled loop each
    [(3 * MiB + 7, "d2d")],                     # past the 96-workgroup clamp: unrolled loop twice, remainder loop, 7-byte tail
    [(3 * MiB + 7, "h2d"), (1, "d2h"), (4095, "d2d"), (64 * 1024 + 9, "d2h")],          # blocks_per_seg from the largest
    [(2 * MiB + 16 * 3 + 5, "d2h"), (17, "h2d")],
]


@pytest.mark.parametrize("segs", COPY_CASES, ids=["-".join("%d%s" % s for s in c) for c in COPY_CASES])
def test_staging_copy_kernel(gpu_ctx, segs):
    """k_mskf_copy (fe_launch_copy: every staging copy of the hot path) on the context's HIP stream: 1 to 6 segments per
    launch, sizes around the 16-byte vector width (1, 15, 16, 17, 4095), a segment that runs the 4-deep unrolled loop, one
    past the 96-workgroup clamp, small and large segments mixed; host -> device, device -> host, device -> device.  Byte
    for byte, and the canary bytes after each destination are untouched."""
    hip = _Hip()
    rng = np.random.default_rng(len(segs) * 1000 + segs[0][0] % 1000)
    try:
        dsts, srcs, sizes, datas, dkinds = [], [], [], [], []
        for n, kind in segs:
            src_pinned, dst_pinned = kind == "h2d", kind == "d2h"
            data = rng.integers(0, 256, n + CANARY, dtype=np.uint8)
            canary = np.full(n + CANARY, 0xA5, np.uint8)
            src = hip.alloc(n + CANARY, src_pinned)
            dst = hip.alloc(n + CANARY, dst_pinned)
            hip.put(src, data)
            hip.put(dst, canary)
            dsts.append(dst); srcs.append(src); sizes.append(n); datas.append(data); dkinds.append(dst_pinned)
        gpu_ctx.sync()
        gpu_ctx.launch_copy(dsts, srcs, sizes)
        gpu_ctx.sync()
        for dst, n, data, (_, kind) in zip(dsts, sizes, datas, segs):
            got = hip.get(dst, n + CANARY)
            bad = np.flatnonzero(got[:n] != data[:n])
            assert bad.size == 0, (kind, n, bad[:8])
            assert (got[n:] == 0xA5).all(), (kind, n, "canary overwritten")
    finally:
        gpu_ctx.sync()
        hip.free()
