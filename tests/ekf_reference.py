"""Plain long-double restatement of the covariance half of the filter's prediction, for the kernel tests.

Written from the published MSCKF equations (Mourikis & Roumeliotis 2007; processModel and stateAugmentation of
msckf_vio.cpp:409-469 and :564-582), not from the device code or the CPU oracle:

  * F (21 x 21) and G (21 x 12) in full, Phi = I + F dt + (F dt)^2 / 2 + (F dt)^3 / 6;
  * Phi(0,0) replaced by R(q_new) R(q_null)^T, then the observability fix-ups A - (A u - w) s^T of the velocity (6..8) and
    position (12..14) rows, both from the un-fixed A;
  * Q = Phi G Qc G^T Phi^T dt with Qc = diag(sigma_g^2, sigma_bg^2, sigma_a^2, sigma_ba^2) (I_3 each);
  * P_II <- Phi P_II Phi^T + Q, P_IC <- Phi P_IC, P_CI <- P_CI Phi^T, symmetrised, once per IMU sample;
  * augmentation: rows / columns [d, d + 6) = J [P_II P_IC], corner J P_II J^T, symmetrised.

Everything is computed in np.longdouble.  `mutate` switches in one deliberate mistake at a time (test_ekf_reference.py
shows that each one moves the result far beyond the GPU tests' bars).

IMU records (`mskf_imu_step`, include/mskf_hip.h) come from `imu_steps`, which integrates a physically consistent
trajectory: JPL quaternions [x y z w], R(q) = world -> body.
"""
import numpy as np

from msckf_stereo_c_amd.ctypes_types import IMU_STEP      # the record layout (37 doubles) only

LD = np.longdouble
N = 21
GRAVITY = np.array([0.0, 0.0, -9.81])

MUTATIONS = ("no_cube", "w2_sign", "phi00_series", "F60_order", "qc_swap")


def skew(v):
    x, y, z = v
    return np.array([[0, -z, y], [z, 0, -x], [-y, x, 0]], dtype=np.asarray(v).dtype)


def rot(q):
    """JPL quaternion [x y z w] -> rotation world -> body: (2w^2 - 1) I - 2w [v]x + 2 v v^T."""
    q = np.asarray(q, dtype=np.float64)
    v, w = q[:3], q[3]
    return (2 * w * w - 1) * np.eye(3) - 2 * w * skew(v) + 2 * np.outer(v, v)


def quat_axis_angle(axis, angle):
    """JPL quaternion of a rotation by `angle` about `axis`."""
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    q = np.concatenate([a * np.sin(angle / 2), [np.cos(angle / 2)]])
    return q / np.linalg.norm(q)


def _quat_step(q, omega, dt):
    """Closed-form zeroth-order JPL integration q <- (cos(|w| dt / 2) I + sin(|w| dt / 2) / |w| Omega(w)) q,
    Omega(w) = [[-[w]x, w], [-w^T, 0]] (Trawny & Roumeliotis, eq. 122)."""
    om = np.zeros((4, 4))
    om[:3, :3] = -skew(omega)
    om[:3, 3] = omega
    om[3, :3] = -np.asarray(omega)
    n = np.linalg.norm(omega)
    if n < 1e-12:
        M = np.eye(4) + 0.5 * dt * om
    else:
        M = np.cos(n * dt / 2) * np.eye(4) + np.sin(n * dt / 2) / n * om
    q = M @ q
    return q / np.linalg.norm(q)


def imu_steps(n_steps, dt, gyro=(0.0, 0.0, 0.0), acc=(0.3, -0.2, 9.9), q0=(0.0, 0.0, 0.0, 1.0), v0=(0.4, -0.1, 0.2),
              p0=(1.0, 2.0, 0.5), gravity=GRAVITY, seed=None, jitter=0.0):
    """`n_steps` mskf_imu_step records of a trajectory driven by body rate `gyro` (rad/s) and specific force `acc` (m/s^2,
    body frame; the default is not the gravity reaction, so the body accelerates and w2 is not zero), from attitude q0.
    jitter > 0 perturbs gyro / acc per step (seeded).  Returns a numpy record array of dtype IMU_STEP."""
    rng = np.random.default_rng(seed)
    g = np.asarray(gravity, dtype=np.float64)
    q = np.asarray(q0, dtype=np.float64) / np.linalg.norm(q0)
    v, p = np.array(v0, dtype=np.float64), np.array(p0, dtype=np.float64)
    out = np.zeros(n_steps, IMU_STEP)
    for k in range(n_steps):
        w = np.asarray(gyro, dtype=np.float64) + (rng.normal(size=3) * jitter if jitter else 0.0)
        a = np.asarray(acc, dtype=np.float64) + (rng.normal(size=3) * jitter if jitter else 0.0)
        q_null, v_null, p_null = q.copy(), v.copy(), p.copy()
        R = rot(q)
        # new nominal state: attitude in closed form, velocity / position with the world acceleration held over the step
        acc_w = R.T @ a + g
        q = _quat_step(q, w, dt)
        v = v_null + acc_w * dt
        p = p_null + v_null * dt + 0.5 * acc_w * dt * dt
        R_null = rot(q_null)
        u = R_null @ g
        r = out[k]
        r["dt"], r["gyro"], r["acc"] = dt, w, a
        r["R_t"] = R.T.reshape(-1)
        r["Phi00"] = (rot(q) @ R_null.T).reshape(-1)
        r["u"], r["s"] = u, u / (u @ u)
        r["w1"] = skew(v_null - v) @ g
        r["w2"] = skew(dt * v_null + p_null - p) @ g
    return out


def qc_of(cfg):
    """Diagonal of the continuous noise covariance per 3-block: gyro, gyro bias, acc, acc bias (an mskf_ekf_cfg)."""
    return np.array([cfg.noise_gyro ** 2, cfg.noise_gyro_bias ** 2, cfg.noise_acc ** 2, cfg.noise_acc_bias ** 2])


def phi_q(step, qc, mutate=None):
    """(Phi, Q) of one IMU record, long double."""
    dt = LD(step["dt"])
    w = np.asarray(step["gyro"], dtype=LD)
    a = np.asarray(step["acc"], dtype=LD)
    Rt = np.asarray(step["R_t"], dtype=LD).reshape(3, 3)
    I3 = np.eye(3, dtype=LD)
    F = np.zeros((N, N), dtype=LD)
    F[0:3, 0:3] = -skew(w)
    F[0:3, 3:6] = -I3
    F[6:9, 0:3] = -(skew(a) @ Rt) if mutate == "F60_order" else -(Rt @ skew(a))
    F[6:9, 9:12] = -Rt
    F[12:15, 6:9] = I3
    G = np.zeros((N, 12), dtype=LD)
    G[0:3, 0:3] = -I3
    G[3:6, 3:6] = I3
    G[6:9, 6:9] = -Rt
    G[9:12, 9:12] = I3
    Fdt = F * dt
    Fdt2 = Fdt @ Fdt
    Phi = np.eye(N, dtype=LD) + Fdt + Fdt2 / 2
    if mutate != "no_cube":
        Phi = Phi + (Fdt2 @ Fdt) / 6
    if mutate != "phi00_series":
        Phi[0:3, 0:3] = np.asarray(step["Phi00"], dtype=LD).reshape(3, 3)
    u = np.asarray(step["u"], dtype=LD)
    s = np.asarray(step["s"], dtype=LD)
    w1 = np.asarray(step["w1"], dtype=LD)
    w2 = np.asarray(step["w2"], dtype=LD) * (-1 if mutate == "w2_sign" else 1)
    A1, A2 = Phi[6:9, 0:3].copy(), Phi[12:15, 0:3].copy()
    Phi[6:9, 0:3] = A1 - np.outer(A1 @ u - w1, s)
    Phi[12:15, 0:3] = A2 - np.outer(A2 @ u - w2, s)
    qd = np.asarray(qc, dtype=LD)
    if mutate == "qc_swap":
        qd = qd[[2, 1, 0, 3]]
    Qc = np.diag(np.repeat(qd, 3))
    Q = Phi @ G @ Qc @ G.T @ Phi.T * dt
    return Phi, Q


def propagate(P, steps, qc, mutate=None):
    """P (d x d) propagated over the IMU records one at a time; returns (P, [Phi_k], [Q_k]) in long double."""
    P = np.array(P, dtype=LD)
    Phis, Qs = [], []
    for st in steps:
        Phi, Q = phi_q(st, qc, mutate)
        Pn = P.copy()
        Pn[:N, :N] = Phi @ P[:N, :N] @ Phi.T + Q
        Pn[:N, N:] = Phi @ P[:N, N:]
        Pn[N:, :N] = P[N:, :N] @ Phi.T
        P = (Pn + Pn.T) / 2
        Phis.append(Phi)
        Qs.append(Q)
    return P, Phis, Qs


def compose(Phis):
    """Phi_n ... Phi_1 (identity for no steps)."""
    T = np.eye(N, dtype=LD)
    for Phi in Phis:
        T = Phi @ T
    return T


def augment(P, J):
    """State augmentation with the 6 x 21 Jacobian J: the new clone's rows / columns appended, symmetrised."""
    P = np.array(P, dtype=LD)
    J = np.asarray(J, dtype=LD)
    d = P.shape[0]
    Pn = np.zeros((d + 6, d + 6), dtype=LD)
    Pn[:d, :d] = P
    Pn[d:, :d] = J @ P[:N, :d]
    Pn[:d, d:] = Pn[d:, :d].T
    Pn[d:, d:] = J @ P[:N, :N] @ J.T
    return (Pn + Pn.T) / 2


def augment_jacobian(rng):
    """A J of the shape stateAugmentation builds: R_i_c at (0,0), I at (0,15), [R^T t]x at (3,0), I at (3,12) and (3,18)."""
    J = np.zeros((6, N))
    J[0:3, 0:3] = rot(quat_axis_angle(rng.normal(size=3), rng.uniform(0, np.pi)))
    J[0:3, 15:18] = np.eye(3)
    J[3:6, 0:3] = skew(rng.normal(size=3) * 0.1)
    J[3:6, 12:15] = np.eye(3)
    J[3:6, 18:21] = np.eye(3)
    return J


def spd(d, rng, scale=1e-3):
    """A symmetric positive definite d x d covariance like ekf_problems.make_problem's."""
    A = rng.normal(size=(d, d))
    P = scale * (A @ A.T / d + np.eye(d))
    return (P + P.T) / 2


def block_errors(got, ref):
    """max |got - ref| / max |ref| of the P_II and P_IC blocks."""
    ref = np.asarray(ref, dtype=LD)
    got = np.asarray(got, dtype=LD)
    out = {}
    for name, sl in (("II", (slice(0, N), slice(0, N))), ("IC", (slice(0, N), slice(N, None)))):
        r = ref[sl]
        if r.size == 0:
            continue
        out[name] = float(np.abs(got[sl] - r).max() / max(np.abs(r).max(), LD(1e-300)))
    return out
