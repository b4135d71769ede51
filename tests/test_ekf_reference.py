"""CPU tests of the long-double prediction reference (ekf_reference.py) the GPU filter tests compare with.

They pin the reference's own algebra (the observability fix-up holds, dt = 0 is the identity, the composed transition
equals the stepwise one) and show that the GPU bars of test_gpu_filter_predict.py have teeth: each deliberate mistake
in MUTATIONS moves Phi, Q or P by at least 1e4 times the bar it would have to get through."""
import numpy as np
import pytest

from msckf_stereo_c_amd.ctypes_types import default_ekf_cfg

import ekf_reference as R

LD = R.LD
QC = R.qc_of(default_ekf_cfg())
# the bars of test_gpu_filter_predict.py
BAR_PHI = 1e-14          # max |dPhi|
BAR_Q = 1e-13            # max |dQ| / max |Q|
BAR_P = 1e-12            # max |dP_blk| / max |P_blk|, P_II and P_IC

ATTITUDES = {"identity": (0.0, 0.0, 0.0, 1.0), "general": R.quat_axis_angle((1.0, 2.0, 3.0), 2.0),
             "near_180": R.quat_axis_angle((0.3, -1.0, 0.5), np.pi - 1e-3)}


@pytest.mark.parametrize("dt", [0.005, 0.02])
@pytest.mark.parametrize("gyro", [(0.0, 0.0, 0.0), (1.0, -2.0, 2.0)])
@pytest.mark.parametrize("att", sorted(ATTITUDES))
def test_observability_fixup(dt, gyro, att):
    """After the fix-up, Phi[6:9, 0:3] u = w1 and Phi[12:15, 0:3] u = w2 (Hesch et al.: the unobservable directions of
    the linearised system stay unobservable)."""
    steps = R.imu_steps(5, dt, gyro=gyro, q0=ATTITUDES[att], seed=3, jitter=0.1)
    for st in steps:
        Phi, _ = R.phi_q(st, QC)
        u = np.asarray(st["u"], dtype=LD)
        for rows, w in ((slice(6, 9), st["w1"]), (slice(12, 15), st["w2"])):
            w = np.asarray(w, dtype=LD)
            err = float(np.abs(Phi[rows, 0:3] @ u - w).max())
            assert err <= 1e-15 * max(1.0, float(np.abs(w).max())), (att, err)


def test_dt_zero_is_identity():
    """dt = 0: Phi = I apart from Phi(0,0) = Phi00 and the fix-up rows (A = 0 there, so they become w s^T); Q = 0."""
    st = R.imu_steps(1, 0.0, gyro=(1.0, 2.0, 3.0), q0=ATTITUDES["general"])[0]
    st["w1"], st["w2"] = (0.5, -0.25, 1.0), (-2.0, 0.125, 0.75)       # not what dt = 0 produces: the fix-up rows must show them
    Phi, Q = R.phi_q(st, QC)
    want = np.eye(21, dtype=LD)
    want[0:3, 0:3] = np.asarray(st["Phi00"], dtype=LD).reshape(3, 3)
    s = np.asarray(st["s"], dtype=LD)
    want[6:9, 0:3] = np.outer(np.asarray(st["w1"], dtype=LD), s)
    want[12:15, 0:3] = np.outer(np.asarray(st["w2"], dtype=LD), s)
    assert np.array_equal(Phi, want)
    assert not Q.any()


@pytest.mark.parametrize("n_steps", [2, 10, 40])
def test_composition_equals_stepwise(n_steps):
    """The device applies Phi_n ... Phi_1 to the clone cross terms once; the reference applies Phi once per step.  At long
    double the two agree to rounding."""
    rng = np.random.default_rng(n_steps)
    d = 21 + 6 * 5
    P0 = R.spd(d, rng)
    steps = R.imu_steps(n_steps, 0.01, gyro=(0.5, -3.0, 1.0), q0=ATTITUDES["general"], seed=n_steps, jitter=0.05)
    P, Phis, _ = R.propagate(P0, steps, QC)
    once = R.compose(Phis) @ np.asarray(P0[:21, 21:], dtype=LD)
    err = float(np.abs(P[:21, 21:] - once).max() / np.abs(once).max())
    assert err < 1e-16, err
    assert np.array_equal(P, P.T)


def _outputs(mutate, steps, P0):
    P, Phis, Qs = R.propagate(P0, steps, QC, mutate)
    return R.compose(Phis[:1]), R.compose(Phis), Qs[0], P


@pytest.mark.parametrize("att", ["general", "near_180"])
@pytest.mark.parametrize("mutation", R.MUTATIONS)
def test_bars_have_teeth(mutation, att):
    """Each mutation of the reference moves Phi (one step or composed), Q or P by at least 1e4 x the GPU test's bar, on
    the data those tests use (dt = 5 ms, |w| = 3 rad/s, an accelerating body, d = 45).  Mutations the data cannot see are
    not listed: the sign or transpose of G's -R^T block cancels in G Qc G^T (each 3 x 3 block of Qc is isotropic), and
    dropping the symmetrisation only changes rounding (the GPU tests check exact symmetry instead)."""
    rng = np.random.default_rng(11)
    P0 = R.spd(45, rng)
    steps = R.imu_steps(10, 0.005, gyro=(0.0, 3.0, 0.0), q0=ATTITUDES[att])
    ok = _outputs(None, steps, P0)
    bad = _outputs(mutation, steps, P0)
    ratios = {
        "Phi1": float(np.abs(bad[0] - ok[0]).max()) / BAR_PHI,
        "PhiN": float(np.abs(bad[1] - ok[1]).max()) / BAR_PHI,
        "Q": float(np.abs(bad[2] - ok[2]).max() / np.abs(ok[2]).max()) / BAR_Q,
    }
    for blk, e in R.block_errors(bad[3], ok[3]).items():
        ratios["P_" + blk] = e / BAR_P
    print(mutation, att, {k: "%.1e" % v for k, v in ratios.items()})
    assert max(ratios.values()) >= 1e4, ratios
