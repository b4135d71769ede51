"""Reference arithmetic of the direct measurement update (k_ekf_direct_update behind mskf_ekf_update_direct*), two ways:

  direct_update_fixed    the arithmetic contract of DESIGN.md section 3, operation by operation in IEEE doubles, every sum in
                         the contract's order: what the device must give bit for bit (P, delta_x, gamma, pos_var, status);
  direct_update_literal  the reference's own measurementUpdate expressions (msckf_vio.cpp:831-904) with R in place of
                         observation_noise * I, in long double: S = H P H^T + R, K = P H^T S^-1 (S inverted by Gauss-Jordan
                         elimination, not by the contract's Cholesky factor), delta_x = K r, (I - K H) P, (X + X^T) / 2.

numpy multiplies and adds element by element, one rounding each, and never contracts a * b + c: a vectorised line below is
the scalar line of the contract for every column at once.

`mutate` of direct_update_fixed switches in one deliberate mistake (test_direct_update_reference.py).
"""
import math

import numpy as np

LD = np.longdouble
N = 21
MAX_ROWS = 6
MUTATIONS = ("no_R", "no_sym", "wrong_block", "dx_sign", "no_back_substitution")


def direct_update_fixed(P, H, r, R, gate=0.0, mutate=None):
    """dict(P, dx, gamma, status, pos_var) of the contract.  status 1 applied, 0 gated out, 2 S not positive definite; unless 1,
    P is returned as given and dx is zero."""
    P = np.array(P, dtype=np.float64)
    H = np.asarray(H, dtype=np.float64).reshape(-1, N)
    r = np.asarray(r, dtype=np.float64).reshape(-1)
    m, d = len(r), P.shape[0]
    R = np.asarray(R, dtype=np.float64).reshape(m, m)
    rows = [(k + 6) % d for k in range(N)] if mutate == "wrong_block" else list(range(N))
    G = np.zeros((m, d))
    for a in range(m):
        g = np.zeros(d)
        for k in range(N):
            g = g + H[a, k] * P[rows[k], :]
        G[a] = g
    S = np.zeros((m, m))
    for a in range(m):
        for b in range(a + 1):
            s = 0.0
            for k in range(N):
                s = s + float(G[a, k]) * float(H[b, k])
            if mutate != "no_R":
                s = s + float(R[a, b])
            S[a, b] = S[b, a] = s
    unchanged = dict(P=P, dx=np.zeros(d), gamma=0.0, status=2, pos_var=np.array([P[12, 12], P[13, 13], P[14, 14]]))
    L = np.zeros((m, m))
    for j in range(m):
        s = float(S[j, j])
        for k in range(j):
            s = s - float(L[j, k]) * float(L[j, k])
        if not s > 0.0:
            return unchanged
        L[j, j] = math.sqrt(s)
        for i in range(j + 1, m):
            t = float(S[i, j])
            for k in range(j):
                t = t - float(L[i, k]) * float(L[j, k])
            L[i, j] = t / float(L[j, j])
    y = np.zeros(m)
    for i in range(m):
        s = float(r[i])
        for k in range(i):
            s = s - float(L[i, k]) * float(y[k])
        y[i] = s / float(L[i, i])
    gamma = 0.0
    for i in range(m):
        gamma = gamma + float(y[i]) * float(y[i])
    if gate > 0.0 and gamma > gate:
        return dict(unchanged, gamma=gamma, status=0)
    W = np.zeros((m, d))
    for i in range(m):
        s = G[i].copy()
        for k in range(i):
            s = s - L[i, k] * W[k]
        W[i] = s / L[i, i]
    if mutate != "no_back_substitution":
        for i in range(m - 1, -1, -1):
            s = W[i].copy()
            for k in range(i + 1, m):
                s = s - L[k, i] * W[k]
            W[i] = s / L[i, i]
    Kt = W
    dx = np.zeros(d)
    for a in range(m):
        dx = dx + Kt[a] * (-r[a] if mutate == "dx_sign" else r[a])
    T = np.zeros((d, d))
    for a in range(m):
        T = T + np.outer(Kt[a], G[a])
    A = P - T
    Pn = A if mutate == "no_sym" else (A + A.T) * 0.5
    return dict(P=Pn, dx=dx, gamma=gamma, status=1, pos_var=np.array([Pn[12, 12], Pn[13, 13], Pn[14, 14]]))


def inverse_ld(S):
    """Inverse of a small matrix in long double: Gauss-Jordan with partial pivoting (numpy.linalg has no long double)."""
    m = S.shape[0]
    A = np.concatenate([np.array(S, dtype=LD), np.eye(m, dtype=LD)], axis=1)
    for c in range(m):
        p = c + int(np.argmax(np.abs(A[c:, c])))
        A[[c, p]] = A[[p, c]]
        A[c] = A[c] / A[c, c]
        for i in range(m):
            if i != c:
                A[i] = A[i] - A[i, c] * A[c]
    return A[:, m:]


def full_H(H, d):
    Hf = np.zeros((H.shape[0], d), dtype=LD)
    Hf[:, :N] = H
    return Hf


def direct_update_literal(P, H, r, R):
    """dict(P, dx, gamma, K, S) in long double, the reference's expressions as written."""
    P = np.array(P, dtype=LD)
    d = P.shape[0]
    r = np.asarray(r, dtype=LD).reshape(-1)
    m = len(r)
    Hf = full_H(np.asarray(H, dtype=LD).reshape(m, N), d)
    R = np.asarray(R, dtype=LD).reshape(m, m)
    S = Hf @ P @ Hf.T + R
    Si = inverse_ld(S)
    K = P @ Hf.T @ Si
    dx = K @ r
    I_KH = np.eye(d, dtype=LD) - K @ Hf
    X = I_KH @ P
    return dict(P=(X + X.T) / 2, dx=dx, gamma=r @ Si @ r, K=K, S=S)


def joseph(P, H, R, K):
    """(I - K H) P (I - K H)^T + K R K^T in long double, symmetrised."""
    P = np.array(P, dtype=LD)
    d = P.shape[0]
    K = np.asarray(K, dtype=LD)
    m = K.shape[1]
    Hf = full_H(np.asarray(H, dtype=LD).reshape(m, N), d)
    I_KH = np.eye(d, dtype=LD) - K @ Hf
    X = I_KH @ P @ I_KH.T + K @ np.asarray(R, dtype=LD).reshape(m, m) @ K.T
    return (X + X.T) / 2


# ---- the distances the bars are in: entries of a covariance over the prior standard deviations of their row and column,
# entries of a correction over the prior standard deviation of their state (a P whose diagonal spans ten decades has no
# single absolute scale)
def cov_distance(Pa, Pb, P_prior):
    sd = np.sqrt(np.diag(np.asarray(P_prior, dtype=LD)))
    return float(np.max(np.abs(np.asarray(Pa, dtype=LD) - np.asarray(Pb, dtype=LD)) / np.outer(sd, sd)))


def dx_distance(xa, xb, P_prior):
    sd = np.sqrt(np.diag(np.asarray(P_prior, dtype=LD)))
    return float(np.max(np.abs(np.asarray(xa, dtype=LD) - np.asarray(xb, dtype=LD)) / sd))


# ---- the P set and the measurements of the tests
DIMS = (21, 27, 63, 69, 201, 405)
ROWS = (1, 3, 6)
P_KINDS = ("spd", "grown", "identity")


def spd_scaled(d, rng):
    """Random SPD with a diagonal spanning 1e-8 .. 1e2: D C D, C a well-conditioned correlation-like matrix, D the standard
    deviations 1e-4 .. 1e1 with both ends present."""
    A = rng.normal(size=(d, d))
    C = A @ A.T / d + np.eye(d)
    sd = 10.0 ** rng.uniform(-4, 1, size=d)
    sd[rng.permutation(d)[:2]] = (1e-4, 1e1)
    P = C * np.outer(sd / np.sqrt(np.diag(C)), sd / np.sqrt(np.diag(C)))
    return (P + P.T) / 2


def grow_inputs(d, seed=7):
    """(P0 21 x 21, [(imu steps, J)] per clone) from which predict / augment calls grow a d-dimensional covariance."""
    import ekf_reference as ER
    rng = np.random.default_rng(seed)
    P0 = ER.spd(N, rng)
    steps = ER.imu_steps(2, 0.005, gyro=(0.1, 0.3, -0.2), q0=ER.quat_axis_angle((1.0, 2.0, 3.0), 0.4), seed=seed, jitter=0.02)
    return P0, [(steps, ER.augment_jacobian(rng)) for _ in range((d - N) // 6)]


def grown_host(d, qc, seed=7):
    """The same growth by the long-double restatement of the prediction (tests/ekf_reference.py), rounded to doubles: the CPU
    tests' stand-in for the covariance the device grows from grow_inputs."""
    import ekf_reference as ER
    P0, seq = grow_inputs(d, seed)
    P = np.array(P0, dtype=LD)
    for steps, J in seq:
        P, _, _ = ER.propagate(P, steps, qc)
        P = ER.augment(P, J)
    P = np.array(P, dtype=np.float64)
    return (P + P.T) / 2


DEFAULT_QC = np.array([0.005 ** 2, 0.001 ** 2, 0.05 ** 2, 0.01 ** 2])     # default_ekf_cfg(): gyro, gyro bias, acc, acc bias


def make_P(kind, d, seed=0):
    if kind == "identity":
        return np.eye(d)
    if kind == "grown":
        return grown_host(d, DEFAULT_QC)
    return spd_scaled(d, np.random.default_rng(1000 + d + seed))


def make_measurement(P, m, dense, rng, first_col=6):
    """(H, r, R): H dense (every IMU column) or a selector of m consecutive columns from first_col (6: velocity, then acc bias;
    12: position); R a full SPD matrix at the scale of H P H^T; r drawn with covariance S, so that gamma is about m."""
    if dense:
        H = rng.normal(size=(m, N))
    else:
        H = np.zeros((m, N))
        H[np.arange(m), first_col + np.arange(m)] = 1.0
    HP = H @ P[:N, :N] @ H.T
    sd = np.sqrt(np.diag(HP)) * 10.0 ** rng.uniform(-1, 0.5, size=m)
    A = rng.normal(size=(m, m))
    C = A @ A.T / m + np.eye(m)
    R = C * np.outer(sd / np.sqrt(np.diag(C)), sd / np.sqrt(np.diag(C)))
    R = (R + R.T) / 2
    S = HP + R
    r = np.linalg.cholesky((S + S.T) / 2) @ rng.normal(size=m)
    return H, r, R


# ---- the stream of the zero-velocity tests (CPU: the separation of its inputs on the oracle; GPU: the run) and their threshold,
# pixels: test_direct_update_reference.py::test_zupt_inputs_separate_on_the_oracle has the figures it rests on
ZUPT_STREAM = dict(seed=0x5EED0095, width=188, height=120, n_static=60, motion_scale=2.0)
ZUPT_TEST_MAX_DISPARITY = 0.1


def small_cfgs():
    """Front-end and filter configuration of that stream: a 15 x 24 detector grid for 188 x 120 images, a 6-clone window."""
    from msckf_stereo_c_amd.ctypes_types import default_ekf_cfg, default_fe_cfg
    fe = default_fe_cfg()
    fe.det_rows, fe.det_cols = 15, 24
    return fe, default_ekf_cfg(max_cam_state_size=6)
