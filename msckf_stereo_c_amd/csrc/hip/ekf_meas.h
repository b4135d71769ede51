// ekf_meas.h — MsckfVio::measurementJacobian (reference msckf_vio.cpp:610-677), stated once: the camera poses of a clone,
// the per-observation 4 x 6 Jacobian H_x with the observability projection A - A u (u^T u)^-1 u^T, and the 4 residuals.
//
// The SAME source is compiled for the device (k_ekf_feature_blocks and k_ekf_pair_blocks, ekf_kernels.hip) and for the CPU
// (MsckfVio::dumpFeatureJacobians, and tests/cpp/ekf_meas_test.cpp, which tests/test_ekf_meas.py holds against the oracle's
// measurementJacobian value for value).  All of it is FP64 without FMA contraction (-ffp-contract=off), so the operation
// order written here IS the arithmetic contract: every sum runs left to right as spelled out.
// H_x and r come back as values (registers on the device) that each caller stores in its own layout; the callers derive
// H_f as the negated columns 3..5 of the projected H_x.
#pragma once
#include "../../../include/mskf_hip.h"

#if defined(__HIPCC__)
#define EM_FN __host__ __device__ __forceinline__
#else
#define EM_FN inline
#endif

namespace ekf {

// ------------------------------------------------------------------------------------ small math (3 x 3 row-major)
EM_FN void quat_to_rot(const double *q, double *R) {
    // JPL: R = (2w^2-1) I - 2w [qv]x + 2 qv qv^T   
    const double x = q[0], y = q[1], z = q[2], w = q[3];
    const double a = 2 * w * w - 1, tw = 2 * w;
    R[0] = a + 2 * x * x;        R[1] = tw * z + 2 * x * y;   R[2] = -tw * y + 2 * x * z;
    R[3] = -tw * z + 2 * y * x;  R[4] = a + 2 * y * y;        R[5] = tw * x + 2 * y * z;
    R[6] = tw * y + 2 * z * x;   R[7] = -tw * x + 2 * z * y;  R[8] = a + 2 * z * z;
}
EM_FN void mat3_mul(const double *A, const double *B, double *C) {
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) C[3 * i + j] = A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j];
}
EM_FN void mat3_vec(const double *A, const double *v, double *o) {
    for (int i = 0; i < 3; ++i) o[i] = A[3 * i] * v[0] + A[3 * i + 1] * v[1] + A[3 * i + 2] * v[2];
}
EM_FN void mat3t_vec(const double *A, const double *v, double *o) {
    for (int i = 0; i < 3; ++i) o[i] = A[i] * v[0] + A[3 + i] * v[1] + A[6 + i] * v[2];
}

// ------------------------------------------------------------------------------------ camera poses of a clone (:612-621, :667)
// R_w_c0 = R(q), R_w_c1 = R_c0_c1 R_w_c0, t_c1_w = p - R_w_c1^T t_c0_c1, Rn = R(q_null); t_c0_w is cam.p itself.
EM_FN void cam_pose(const mskf_clone_state &cam, const double *R_c0_c1, const double *t_c0_c1, double R_w_c0[9], double R_w_c1[9], double t_c1_w[3],
                    double Rn[9]) {
    double tmp[3];
    quat_to_rot(cam.q, R_w_c0);
    mat3_mul(R_c0_c1, R_w_c0, R_w_c1);
    mat3t_vec(R_w_c1, t_c0_c1, tmp);
    for (int i = 0; i < 3; ++i) t_c1_w[i] = cam.p[i] - tmp[i];
    quat_to_rot(cam.q_null, Rn);
}

// ------------------------------------------------------------------------------------ one observation
// The feature in the two camera frames: p_c0 = R_w_c0 (p - t_c0_w), p_c1 = R_w_c1 (p - t_c1_w)  (:623-624)
EM_FN void meas_cam_points(const double *R_w_c0, const double *R_w_c1, const double *t_c0_w, const double *t_c1_w, const double *pos, double p_c0[3],
                           double p_c1[3]) {
    const double dp0[3] = {pos[0] - t_c0_w[0], pos[1] - t_c0_w[1], pos[2] - t_c0_w[2]};
    const double dp1[3] = {pos[0] - t_c1_w[0], pos[1] - t_c1_w[1], pos[2] - t_c1_w[2]};
    mat3_vec(R_w_c0, dp0, p_c0);
    mat3_vec(R_w_c1, dp1, p_c1);
}

// The un-projected Jacobian A = dz_dpc0 dpc0_dxc + dz_dpc1 dpc1_dxc (:626-655)
EM_FN void meas_unprojected(const double *R_w_c0, const double *R_w_c1, const double *R_c0_c1, const double p_c0[3], const double p_c1[3], double A[4][6]) {
    // dz_dpc0 (rows 0,1), dz_dpc1 (rows 2,3)
    const double dz[4][3] = {{1 / p_c0[2], 0, -p_c0[0] / (p_c0[2] * p_c0[2])},
                             {0, 1 / p_c0[2], -p_c0[1] / (p_c0[2] * p_c0[2])},
                             {1 / p_c1[2], 0, -p_c1[0] / (p_c1[2] * p_c1[2])},
                             {0, 1 / p_c1[2], -p_c1[1] / (p_c1[2] * p_c1[2])}};
    // dpc0_dxc = [skew(p_c0), -R_w_c0], dpc1_dxc = [R_c0_c1 skew(p_c0), -R_w_c1]
    const double sk[9] = {0, -p_c0[2], p_c0[1], p_c0[2], 0, -p_c0[0], -p_c0[1], p_c0[0], 0};
    double Rsk[9];
    mat3_mul(R_c0_c1, sk, Rsk);
    for (int rr = 0; rr < 4; ++rr) {
        const double *L = rr < 2 ? sk : Rsk;
        const double *Rm = rr < 2 ? R_w_c0 : R_w_c1;
        for (int c = 0; c < 3; ++c) {
            A[rr][c] = dz[rr][0] * L[c] + dz[rr][1] * L[3 + c] + dz[rr][2] * L[6 + c];
            A[rr][3 + c] = -(dz[rr][0] * Rm[c] + dz[rr][1] * Rm[3 + c] + dz[rr][2] * Rm[6 + c]);
        }
    }
}

// The observability constraint (:666-671): Hx = A - A u (u^T u)^-1 u^T with u = [R(q_null) g ; skew(p - p_null) g]
EM_FN void meas_project(const double A[4][6], const double *Rn, const double *p_null, const double *pos, const double *g, double Hx[4][6]) {
    double u[6];
    mat3_vec(Rn, g, u);
    const double dn[3] = {pos[0] - p_null[0], pos[1] - p_null[1], pos[2] - p_null[2]};
    u[3] = dn[1] * g[2] - dn[2] * g[1]; u[4] = dn[2] * g[0] - dn[0] * g[2]; u[5] = dn[0] * g[1] - dn[1] * g[0];
    double uu = 0;
    for (int k = 0; k < 6; ++k) uu += u[k] * u[k];
    for (int rr = 0; rr < 4; ++rr) {
        double Au = 0;
        for (int k = 0; k < 6; ++k) Au += A[rr][k] * u[k];
        for (int c = 0; c < 6; ++c) Hx[rr][c] = A[rr][c] - Au * (1.0 / uu) * u[c];
    }
}

// measurementJacobian of the observation z of the feature at `pos` from the clone `cam`, whose poses (the four arrays after
// `cam`, in cam_pose's order) cam_pose gave: the projected H_x and the residual r = z - h(p) (:673-676).
EM_FN void meas_jacobian(const mskf_clone_state &cam, const double *R_w_c0, const double *R_w_c1, const double *t_c1_w, const double *Rn,
                         const double *R_c0_c1, const double *pos, const double *g, const double *z, double Hx[4][6], double r[4]) {
    double p_c0[3], p_c1[3], A[4][6];
    meas_cam_points(R_w_c0, R_w_c1, cam.p, t_c1_w, pos, p_c0, p_c1);
    meas_unprojected(R_w_c0, R_w_c1, R_c0_c1, p_c0, p_c1, A);
    meas_project(A, Rn, cam.p_null, pos, g, Hx);
    r[0] = z[0] - p_c0[0] / p_c0[2];
    r[1] = z[1] - p_c0[1] / p_c0[2];
    r[2] = z[2] - p_c1[0] / p_c1[2];
    r[3] = z[3] - p_c1[1] / p_c1[2];
}

}  // namespace ekf
#undef EM_FN
