"""Reference arithmetic of the published odometry covariance (msckf_vio.cpp:1262-1293), two ways:

  odom_cov_fixed    the arithmetic contract of DESIGN.md section 3, operation by operation in IEEE doubles: what the device
                    must give bit for bit;
  odom_cov_literal  the reference's own expressions, H_pose * P_imu_pose * H_pose^T on the assembled 6 x 6 matrices and
                    H_vel * P_imu_vel * H_vel^T, in long double.  Written from the reference, not from the device code.

R is the rotation of IMUState::T_imu_body, the INVERSE of the calibration's T_imu_body (msckf_vio.cpp:124-125).
"""
import copy

import numpy as np

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)


def rotation(axis, angle):
    """Rodrigues: rotation by `angle` about `axis`."""
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def calib_with_imu_body(calib, R_file, t=(0.0, 0.0, 0.0)):
    """A copy of `calib` whose T_imu_body (as the calibration file holds it) is [R_file t; 0 1]."""
    c = copy.deepcopy(calib)
    T = np.eye(4)
    T[:3, :3] = R_file
    T[:3, 3] = t
    c.T_imu_body[:] = list(T.reshape(-1))
    return c


def body_rotation(calib):
    """Rotation of IMUState::T_imu_body: the calibration's matrix inverted (:124-125), i.e. its rotation transposed."""
    return np.ascontiguousarray(np.array(calib.T_imu_body, dtype=np.float64).reshape(4, 4)[:3, :3].T)


def _rot_block_fixed(B, R):
    out = np.empty((3, 3))
    for i in range(3):
        M = [(R[i, 0] * B[0, b] + R[i, 1] * B[1, b]) + R[i, 2] * B[2, b] for b in range(3)]
        for j in range(3):
            out[i, j] = (M[0] * R[j, 0] + M[1] * R[j, 1]) + M[2] * R[j, 2]
    return out


# where each 3 x 3 block of the pose covariance comes from: (row offset, column offset) in P, position first (:1269-1273)
POSE_BLOCKS = {(0, 0): (12, 12), (0, 3): (12, 0), (3, 0): (0, 12), (3, 3): (0, 0)}


def odom_cov_fixed(P, R, blocks=POSE_BLOCKS, vel=6, rotate=True):
    """(pose 6 x 6, twist 3 x 3, pos_var 3) in the fixed order of the contract.  The keyword arguments exist for the mutation
    test only: other source blocks, another velocity block, no rotation at all."""
    P = np.asarray(P, dtype=np.float64)
    R = np.asarray(R, dtype=np.float64)

    def f(B):
        return _rot_block_fixed(B, R) if rotate else np.array(B, dtype=np.float64)
    pose = np.empty((6, 6))
    for (r, c), (pr, pc) in blocks.items():
        pose[r:r + 3, c:c + 3] = f(P[pr:pr + 3, pc:pc + 3])
    twist = f(P[vel:vel + 3, vel:vel + 3])
    return pose, twist, np.array([P[12, 12], P[13, 13], P[14, 14]])


def odom_cov_literal(P, R):
    """The reference, literally, in long double: P_imu_pose = [P_pp P_po; P_op P_oo], H_pose = diag(R, R),
    P_body_pose = H_pose P_imu_pose H_pose^T (:1263-1279); P_body_vel = R P[6:9, 6:9] R^T (:1288-1290)."""
    P = np.asarray(P, dtype=LD)
    R = np.asarray(R, dtype=LD)
    P_oo, P_op, P_po, P_pp = P[0:3, 0:3], P[0:3, 12:15], P[12:15, 0:3], P[12:15, 12:15]
    P_imu_pose = np.zeros((6, 6), dtype=LD)
    P_imu_pose[0:3, 0:3] = P_pp
    P_imu_pose[0:3, 3:6] = P_po
    P_imu_pose[3:6, 0:3] = P_op
    P_imu_pose[3:6, 3:6] = P_oo
    H_pose = np.zeros((6, 6), dtype=LD)
    H_pose[0:3, 0:3] = R
    H_pose[3:6, 3:6] = R
    P_body_pose = H_pose @ P_imu_pose @ H_pose.T
    P_body_vel = R @ P[6:9, 6:9] @ R.T
    return P_body_pose, P_body_vel, np.array([P[12, 12], P[13, 13], P[14, 14]], dtype=LD)


def error_bar(P, R):
    """Entry-wise bound 8 eps (|R| |B| |R|^T)_ij for pose and twist: two nested 3-term dot products give gamma_6 ~ 6 eps,
    the rest is room for the long-double side."""
    aP = np.abs(np.asarray(P, dtype=np.float64))
    aR = np.abs(np.asarray(R, dtype=np.float64))
    H = np.zeros((6, 6))
    H[0:3, 0:3] = aR
    H[3:6, 3:6] = aR
    Pp = np.block([[aP[12:15, 12:15], aP[12:15, 0:3]], [aP[0:3, 12:15], aP[0:3, 0:3]]])
    return 8 * EPS * (H @ Pp @ H.T), 8 * EPS * (aR @ aP[6:9, 6:9] @ aR.T)


def as_record(pose, twist, pos_var):
    """The three parts as one row of 48 doubles in the layout of mskf_odom_cov."""
    return np.concatenate([np.asarray(pose, dtype=np.float64).reshape(-1), np.asarray(twist, dtype=np.float64).reshape(-1),
                           np.asarray(pos_var, dtype=np.float64).reshape(-1)])
