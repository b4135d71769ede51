"""Plain long-double restatement of the measurement update's per-feature stage, for the kernel tests.

Written from the published procedure (Feature::initializePosition / jacobian / generateInitialGuess of feature.hpp:192-450;
measurementJacobian, featureJacobian and gatingTest of msckf_vio.cpp:610-677, :735-766, :909-935; measurementUpdate), not
from the device code or the CPU oracle:

  * triangulation: the stereo measurements of the n_init clones as 2 n_init views (cam0, cam1 = cam0 * T_cam0_cam1^-1), every
    pose taken relative to the first cam0; initial depth from the first measurement and the last view; Levenberg-Marquardt on
    (alpha, beta, rho) with the Huber weight sqrt(2 * 0.01 / e) applied SQUARED to J^T J and J^T r, lambda from 1e-3 in
    [1e-10, 1e12] scaled by 10, at most 10 inner and 10 outer iterations counted `do ... while (n++ < 10 && ...)` (so up to
    eleven passes each), stopping at |delta| <= 5e-7; a (A + lambda I) that is not positive definite gives a zero step; the
    result is valid when the point lies in front of every one of the 2 n_init views;
  * per observation H_x = dz/dp_c0 dp_c0/dx + dz/dp_c1 dp_c1/dx (4 x 6), projected as A - A u (u^T u)^-1 u^T with
    u = [R(q_null) g; [p_w - p_null]x g], H_f = -H_x[:, 3:6], r = z - z_hat;
  * the left null space of the stacked H_f through three Householder reflectors (gamma does not depend on the basis);
  * gamma = r_o^T (H_o P H_o^T + sigma^2 I)^-1 r_o, a feature passes when gamma < chi2[dof];
  * update: delta_x = P H^T S^-1 r, P' = P - P H^T S^-1 H P, symmetrised (no compression: it changes nothing in exact
    arithmetic).

Everything is computed in np.longdouble; np.linalg does not keep long double, so the Householder reflectors, the Cholesky
factorisation and the triangular solves are written out here, vectorised per column.  `mutate` switches in one deliberate
mistake at a time (test_feature_cases.py shows that each one moves its output beyond the GPU tests' bars).

Conventions (tests/ekf_problems.py): clones[i] = [q p q_null p_null], JPL quaternions [x y z w], R(q) = world -> cam0;
calib.T_cam1_cam0 = (R01, t01) takes cam0 coordinates to cam1 coordinates, p_c1 = R01 p_c0 + t01 (the reference's
CAMState::T_cam0_cam1).
"""
import os
import re

import numpy as np

LD = np.longdouble
HAVE_LONG_DOUBLE = bool(np.finfo(np.longdouble).eps < 1e-18)
NEED_LONG_DOUBLE = "np.longdouble is not wider than double on this platform (eps %.1e)" % float(np.finfo(np.longdouble).eps)

MUTATIONS = ("huber_not_squared", "valid_cam0_only", "cam1_T_not_inverted", "no_projection", "no_sigma", "dof_off_by_one")

HUBER_EPSILON = LD("0.01")
ESTIMATION_PRECISION = LD("5e-7")
LAMBDA_MIN, LAMBDA_MAX = LD("1e-10"), LD("1e12")


def chi2_table():
    """chi2[dof] for dof 1..99 as the filter tabulates it (ppf 0.05, include/mskf_chi2_table.h); chi2[0] is unused."""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mskf_chi2_table.h")
    with open(path) as f:
        text = f.read()
    body = re.search(r"mskf_chi2_ppf05\[99\] = \{(.*?)\}", text, re.S).group(1)
    vals = [float(v) for v in body.replace("\n", " ").split(",") if v.strip()]
    assert len(vals) == 99
    return np.array([0.0] + vals)


def skew(v):
    x, y, z = v
    return np.array([[0, -z, y], [z, 0, -x], [-y, x, 0]], dtype=LD)


def rot(q):
    """JPL quaternion [x y z w] -> rotation world -> body: (2w^2 - 1) I - 2w [v]x + 2 v v^T."""
    q = np.asarray(q, dtype=LD)
    v, w = q[:3], q[3]
    return (2 * w * w - 1) * np.eye(3, dtype=LD) - 2 * w * skew(v) + 2 * np.outer(v, v)


def _extrinsics(calib):
    T = np.array(calib.T_cam1_cam0, dtype=LD).reshape(4, 4)
    return T[:3, :3], T[:3, 3]


# ------------------------------------------------------------------------------------------------ small dense algebra
def cholesky(A):
    """Lower Cholesky factor of a symmetric positive definite matrix, None when a pivot is not positive."""
    A = np.asarray(A, dtype=LD)
    n = A.shape[0]
    L = np.zeros((n, n), dtype=LD)
    for k in range(n):
        dk = A[k, k] - L[k, :k] @ L[k, :k]
        if not dk > 0:
            return None
        L[k, k] = np.sqrt(dk)
        if k + 1 < n:
            L[k + 1:, k] = (A[k + 1:, k] - L[k + 1:, :k] @ L[k, :k]) / L[k, k]
    return L


def forward_solve(L, B):
    """L^-1 B for a lower triangular L; B is a vector or a matrix."""
    B = np.asarray(B, dtype=LD)
    Y = np.zeros_like(B)
    for k in range(L.shape[0]):
        Y[k] = (B[k] - L[k, :k] @ Y[:k]) / L[k, k]
    return Y


def householder_apply(Hf, X):
    """Q^T X for the Householder QR Hf = Q R of a tall matrix: Hf's columns are annihilated one reflector at a time and
    every reflector is applied to X as well.  Rows Hf.shape[1].. of the result are A^T X for an orthonormal basis A of the
    left null space of Hf."""
    Hf = np.array(Hf, dtype=LD)
    X = np.array(X, dtype=LD)
    for k in range(Hf.shape[1]):
        x = Hf[k:, k]
        nrm = np.sqrt(x @ x)
        if nrm == 0:
            continue
        v = x.copy()
        v[0] += nrm if x[0] >= 0 else -nrm
        beta = 2 / (v @ v)
        Hf[k:, k:] -= np.outer(v, beta * (v @ Hf[k:, k:]))
        X[k:] -= np.outer(v, beta * (v @ X[k:]))
    return X


# ------------------------------------------------------------------------------------------------ triangulation
def _views(calib, clones, obs_clone, obs_z, mutate):
    """(R, t, z) of the 2 n_init views relative to the first cam0 pose, and that pose (camera -> world)."""
    R01, t01 = _extrinsics(calib)
    if mutate == "cam1_T_not_inverted":
        Ri, ti = R01, t01
    else:
        Ri, ti = R01.T, -(R01.T @ t01)            # T^-1
    poses, zs = [], []
    for ci, z in zip(obs_clone, np.asarray(obs_z, dtype=LD).reshape(-1, 4)):
        c = np.asarray(clones[int(ci)], dtype=LD)
        R0, p0 = rot(c[0:4]).T, c[4:7]            # cam0 -> world
        poses.append((R0, p0))
        poses.append((R0 @ Ri, R0 @ ti + p0))     # cam1 -> world = cam0_pose * T^-1
        zs.append(z[0:2])
        zs.append(z[2:4])
    Rw, tw = poses[0]
    R = np.stack([Rc.T @ Rw for Rc, _ in poses])               # pose^-1 * T_c0_w
    t = np.stack([Rc.T @ (tw - tc) for Rc, tc in poses])
    return R, t, np.stack(zs), Rw, tw


def _project(R, t, x):
    return R @ np.array([x[0], x[1], LD(1)], dtype=LD) + x[2] * t


def _cost(R, t, z, x):
    h = _project(R, t, x)
    d = h[:, :2] / h[:, 2:3] - z
    return (d * d).sum()


def triangulate(calib, clones, obs_clone, obs_z, mutate=None):
    """Feature::initializePosition over the observations (obs_clone[k], obs_z[k]) -> dict(position (world), solution
    (alpha, beta, rho) in the first clone's cam0 frame, valid, counters: huber = Huber-weighted measurements over all
    linearisations, rejected = LM steps that did not reduce the cost, outer = outer iterations, failed = 3 x 3 solves
    that were not positive definite)."""
    R, t, z, Rw, tw = _views(calib, clones, obs_clone, obs_z, mutate)
    one = LD(1)
    # initial guess: depth along the first measurement's ray that best explains the last view's measurement
    m = R[-1] @ np.array([z[0, 0], z[0, 1], one], dtype=LD)
    A = np.array([m[0] - z[-1, 0] * m[2], m[1] - z[-1, 1] * m[2]], dtype=LD)
    b = np.array([z[-1, 0] * t[-1, 2] - t[-1, 0], z[-1, 1] * t[-1, 2] - t[-1, 1]], dtype=LD)
    depth = (A @ b) / (A @ A)
    p = np.array([z[0, 0] * depth, z[0, 1] * depth, depth], dtype=LD)
    sol = np.array([p[0] / p[2], p[1] / p[2], one / p[2]], dtype=LD)

    lam = LD("1e-3")
    counters = dict(huber=0, rejected=0, outer=0, failed=0)
    total = _cost(R, t, z, sol)
    W = np.stack([R[:, :, 0], R[:, :, 1], t], axis=2)           # W[m] = [R(:, 0) R(:, 1) t]
    outer = 0
    delta_norm = LD(0)
    while True:
        counters["outer"] += 1
        h = _project(R, t, sol)
        h1, h2, h3 = h[:, 0:1], h[:, 1:2], h[:, 2:3]
        J0 = W[:, 0, :] / h3 - h1 / (h3 * h3) * W[:, 2, :]
        J1 = W[:, 1, :] / h3 - h2 / (h3 * h3) * W[:, 2, :]
        r = h[:, :2] / h3 - z
        e = np.sqrt((r * r).sum(1))
        heavy = e > HUBER_EPSILON
        w = np.where(heavy, np.sqrt(2 * HUBER_EPSILON / np.where(heavy, e, one)), one)
        ws = w if mutate == "huber_not_squared" else w * w
        counters["huber"] += int(heavy.sum())
        Am = np.einsum("m,mi,mj->ij", ws, J0, J0) + np.einsum("m,mi,mj->ij", ws, J1, J1)
        bv = (ws[:, None] * (J0 * r[:, 0:1] + J1 * r[:, 1:2])).sum(0)
        inner = 0
        while True:
            L = cholesky(Am + lam * np.eye(3, dtype=LD))
            if L is None:
                counters["failed"] += 1
                delta = np.zeros(3, dtype=LD)
            else:
                y = forward_solve(L, bv)
                delta = forward_solve(L.T[::-1, ::-1], y[::-1])[::-1]      # back substitution
            new = sol - delta
            delta_norm = np.sqrt(delta @ delta)
            new_cost = _cost(R, t, z, new)
            if new_cost < total:
                reduced = True
                sol, total = new, new_cost
                lam = max(lam / 10, LAMBDA_MIN)
            else:
                reduced = False
                counters["rejected"] += 1
                lam = min(lam * 10, LAMBDA_MAX)
            again = inner < 10 and not reduced
            inner += 1
            if not again:
                break
        again = outer < 10 and delta_norm > ESTIMATION_PRECISION
        outer += 1
        if not again:
            break
    fp = np.array([sol[0] / sol[2], sol[1] / sol[2], one / sol[2]], dtype=LD)
    depth_of_view = (R @ fp + t)[:, 2]
    if mutate == "valid_cam0_only":
        depth_of_view = depth_of_view[0::2]
    return dict(position=Rw @ fp + tw, solution=sol, valid=bool((depth_of_view > 0).all()), counters=counters)


def to_inverse_depth(clones, first_clone, position):
    """World position -> (alpha, beta, rho) in the cam0 frame of clone `first_clone`."""
    c = np.asarray(clones[int(first_clone)], dtype=LD)
    p = rot(c[0:4]) @ (np.asarray(position, dtype=LD) - c[4:7])
    return np.array([p[0] / p[2], p[1] / p[2], 1 / p[2]], dtype=LD)


# ------------------------------------------------------------------------------------------------ Jacobians and gate
def measurement_jacobian(calib, clone, position, z, gravity, mutate=None):
    """(H_x 4 x 6, H_f 4 x 3, r[4]) of one stereo observation."""
    R01, t01 = _extrinsics(calib)
    c = np.asarray(clone, dtype=LD)
    pw = np.asarray(position, dtype=LD)
    g = np.asarray(gravity, dtype=LD)
    Rw0, t0 = rot(c[0:4]), c[4:7]
    Rw1 = R01 @ Rw0
    t1 = t0 - Rw1.T @ t01
    p0 = Rw0 @ (pw - t0)
    p1 = Rw1 @ (pw - t1)
    dz0 = np.zeros((4, 3), dtype=LD)
    dz1 = np.zeros((4, 3), dtype=LD)
    dz0[0, 0] = dz0[1, 1] = 1 / p0[2]
    dz0[0, 2], dz0[1, 2] = -p0[0] / (p0[2] * p0[2]), -p0[1] / (p0[2] * p0[2])
    dz1[2, 0] = dz1[3, 1] = 1 / p1[2]
    dz1[2, 2], dz1[3, 2] = -p1[0] / (p1[2] * p1[2]), -p1[1] / (p1[2] * p1[2])
    A = dz0 @ np.hstack([skew(p0), -Rw0]) + dz1 @ np.hstack([R01 @ skew(p0), -Rw1])
    if mutate == "no_projection":
        Hx = A
    else:
        u = np.concatenate([rot(c[7:11]) @ g, skew(pw - c[11:14]) @ g])
        Hx = A - np.outer(A @ u, u) / (u @ u)
    zhat = np.array([p0[0] / p0[2], p0[1] / p0[2], p1[0] / p1[2], p1[1] / p1[2]], dtype=LD)
    return Hx, -Hx[:, 3:6], np.asarray(z, dtype=LD) - zhat


def feature_gate(calib, clones, P, position, obs_clone, obs_z, gravity, sigma2, mutate=None):
    """featureJacobian + the gate's quadratic form of one feature -> dict(gamma, H_o (4 n_obs - 3) x d, r_o).
    gamma is None when the gate matrix is not positive definite."""
    obs_clone = [int(c) for c in obs_clone]
    obs_z = np.asarray(obs_z, dtype=LD).reshape(-1, 4)
    M = len(obs_clone)
    d = np.asarray(P).shape[0]
    X = np.zeros((4 * M, 6 * M + 1), dtype=LD)            # [H_xj (the observed clones' columns) | r_j]
    Hf = np.zeros((4 * M, 3), dtype=LD)
    for k, ci in enumerate(obs_clone):
        hx, hf, r = measurement_jacobian(calib, clones[ci], position, obs_z[k], gravity, mutate)
        X[4 * k:4 * k + 4, 6 * k:6 * k + 6] = hx
        X[4 * k:4 * k + 4, 6 * M] = r
        Hf[4 * k:4 * k + 4] = hf
    Xo = householder_apply(Hf, X)[3:]
    cols = np.concatenate([21 + 6 * ci + np.arange(6) for ci in obs_clone])
    Hc, ro = Xo[:, :6 * M], Xo[:, 6 * M]
    Ho = np.zeros((4 * M - 3, d), dtype=LD)
    Ho[:, cols] = Hc                                      # (the observed clones are distinct)
    # H_o P H_o^T = A^T (H_xj P H_xj^T) A: H_xj is block diagonal over the observed clones' columns, so the inner product is
    # formed block by block (4 x 6 . 6 x 6 . 6 x 4) and the reflectors then act on its rows and on its columns
    Pcc = np.asarray(P, dtype=LD)[np.ix_(cols, cols)].reshape(M, 6, M, 6)
    hx = np.stack([X[4 * k:4 * k + 4, 6 * k:6 * k + 6] for k in range(M)])
    Mm = np.einsum("aiu,aubv->aibv", hx, Pcc)
    Mm = np.einsum("aibv,bjv->aibj", Mm, hx).reshape(4 * M, 4 * M)
    S = householder_apply(Hf, householder_apply(Hf, Mm).T).T[3:, 3:]
    S = (S + S.T) / 2
    if mutate != "no_sigma":
        S = S + LD(sigma2) * np.eye(4 * M - 3, dtype=LD)
    L = cholesky(S)
    gamma = None
    if L is not None:
        y = forward_solve(L, ro)
        gamma = y @ y
    return dict(gamma=gamma, H_o=Ho, r_o=ro)


def passes(gamma, n_obs, dof_offset, chi2, mutate=None):
    """The gate's verdict: dof = n_obs + dof_offset (-1 for lost features, 0 in the pruning update)."""
    dof = n_obs + dof_offset + (1 if mutate == "dof_off_by_one" else 0)
    return gamma is not None and 1 <= dof < 100 and bool(gamma < chi2[dof])


def update(P, blocks, sigma2):
    """measurementUpdate without compression over blocks = [(H_o, r_o), ...] -> (delta_x, P'), long double."""
    P = np.asarray(P, dtype=LD)
    H = np.vstack([np.asarray(b[0], dtype=LD) for b in blocks])
    r = np.concatenate([np.asarray(b[1], dtype=LD) for b in blocks])
    HP = H @ P
    S = HP @ H.T + LD(sigma2) * np.eye(H.shape[0], dtype=LD)
    L = cholesky((S + S.T) / 2)
    Y = forward_solve(L, HP)                              # L^-1 H P: P H^T S^-1 H P = Y^T Y, P H^T S^-1 r = Y^T L^-1 r
    dx = Y.T @ forward_solve(L, r)
    Pn = P - Y.T @ Y
    return dx, (Pn + Pn.T) / 2
