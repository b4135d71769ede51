// ekf_device.h — device-side descriptors of the MSCKF measurement-update kernels and, defined here (the plain numbers: ekf_limits.h) and
// nowhere else, what the host (mskf_capi_ekf.cpp) and the kernels must agree on: the limits a stream is routed by, the route bits, the
// mode predicates, the rows_out record, the launchers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../../include/mskf_hip.h"
#include "ekf_limits.h"      // the limits, the compression modes and the rows_out record: plain C++, tested on the CPU

#define EKF_SLOTS 64          // feature workgroups per stream and launch (each loops over its features)

// ---- EkfStreamDev::route: which kernels handle a stream's update, decided per STREAM from its own features (never from
// the rest of the batch, so a stream's arithmetic does not depend on its neighbours)
#define EKF_ROUTE_PAIRS 1         // pair kernels: every feature has exactly the same two Jacobian clones (the pruning update)
#define EKF_ROUTE_WAVE 2          // wave-per-feature class: every feature <= FEAT_WAVE_CLONES observations, triangulation <= TRI_SMALL_CLONES clones
#define EKF_ROUTE_SMALL 4         // whole update in k_ekf_small_update (<= SU_MAX_NA active columns possible); the general kernels leave it alone
enum { GM_GRAM = 0, GM_T = 1, GM_S2 = 2, GM_PUPD = 3 };      // ekf_launch_gemm's mode

// Per feature of one update (device copy of mskf_ekf_feature + row offset of its block)
struct EkfFeatDev {
    int obs_start, n_obs;
    int needs_init, init_start, n_init;
    int row_off;              // first row of this feature's (4 n_obs - 3)-row block in Hs
    double position[3];
    unsigned long long colmask;   // device: bit c set = the block carries clone c's six columns and is stacked (0 = not stacked)
};

// Everything the update kernels need for one VIO stream.
struct EkfStreamDev {
    double *P;                // ld x ld, row-major, only [0,d) x [0,d) is live
    int d, ld;
    int n_clones, n_feat, n_obs;
    int dof_offset, apply_row_cap, max_stack_rows;
    int m_total;              // sum of block rows of all features
    double sigma2;            // Feature::observation_noise (variance)
    double gravity[3];
    double R_c0_c1[9], t_c0_c1[3];       // CAMState::T_cam0_cam1
    double R_imu_body[9];                // rotation of IMUState::T_imu_body = inverse of mskf_calib.T_imu_body (msckf_vio.cpp:124-125), row-major; k_ekf_odom_cov
    const double *chi2;                  // table[100], index = dof
    const mskf_clone_state *clones;      // n_clones
    EkfFeatDev *feats;                   // n_feat
    const int *obs_clone;                // n_obs
    const double *obs_z;                 // n_obs x 4
    // m_total x ld stacked (null-space projected) Jacobian.  A block is written only in the columns of the clones its
    // feature observed (+ column d, the residual); what a row carries is its rowmask (clone bits, 0 = the row is not
    // stacked: failed triangulation / gate, or behind the row cap).  Nothing else of a row is ever written or read.
    double *Hs;
    unsigned long long *rowmask;   // m_total, written by the feature kernels for their own rows
    // The dense update works on the active columns only (compact index i <-> column act[i]): a stacked Jacobian is
    // identically zero in the 21 IMU columns and in the columns of clones none of its features observed, and such
    // columns contribute nothing to S, K or the covariance downdate.
    double *T;                // na x (d+1) work: T = R P[act, :], then Y = L^-1 [T | Q^T r]
    double *S;                // (na+1)^2 work (compact): Gram matrix [H_act|r]^T [H_act|r], then its Cholesky factor L = R^T (+ the Q^T r row)
    double *W;                // na x na work (compact): S = T[:, act] R^T + sigma^2 I, then its Cholesky factor
    int *act;                 // active columns of this update (the 6 columns of every clone a stacked feature observed), ascending; count in rows_out[EKF_ROWS_NA];
                              // act + ld: indices of the stacked rows, in order, when the update is not compressed (2 ld ints in all)
    double *gate_S;           // EKF_SLOTS x (nmax x nmax)
    int nmax;                 // 4 * max_clones
    double *delta_x;          // d
    uint8_t *feat_status;     // n_feat: bit0 triangulation valid, bit1 gate passed and stacked
    double *gamma;            // n_feat
    double *pos_out;          // n_feat x 3: feature positions used (triangulated when needs_init)
    double *pos_var_out;      // 3: P(12,12), P(13,13), P(14,14) after the update (epilogue of k_ekf_gemm<PUPD>), or null
    int route;                // EKF_ROUTE_* bits, set by the host
    int na_max;               // 6 x the clones any feature of this update observed: an upper bound of the active columns (from the host)
    int qr_mode;              // mskf_ekf_cfg.compression_mode: 0 auto (Gram + Cholesky, Householder TSQR when flagged), 1 Gram only, 2 TSQR always,
                              // 3 the reference's own rule (Householder when rows > columns, uncompressed otherwise)
    const int *tri_idx;       // features that need triangulation (pair path: k_ekf_triangulate), n_tri of them
    int n_tri;
    int *rows_out;            // EKF_ROWS_COUNT ints, slots EKF_ROWS_* (ekf_limits.h)
    // propagation / augmentation
    const double *PhiQ;       // n_steps x (2 x 21 x 21): Phi then Q   (generic form)
    const mskf_imu_step *imu_steps;   // or: n_steps compact IMU records, Phi/Q formed on the device
    double qc[4];             // continuous noise variances: gyro, gyro bias, acc, acc bias (msckf_vio.cpp:174-178)
    int n_steps;
    const double *J;          // 6 x 21
    int remove_index;         // clone to delete (-1 = none)
    int remove_index2;        // second clone to delete, > remove_index (-1 = none)
    double *P_dst;            // destination of the out-of-place clone removal
};

// One stream of a direct-update batch (k_ekf_direct_update, ekf_direct.hip): m rows H r R on the IMU block, P updated in place.
struct EkfDirectDev {
    double *P;                // ld x ld, row-major, [0,d) x [0,d) live
    int d, ld;
    int m;                    // 0: the stream takes no part
    int *status;              // out: 1 applied, 0 gated out, 2 S not positive definite (P untouched unless 1)
    const double *H;          // m x 21
    const double *r;          // m
    const double *R;          // m x m, symmetric
    double gate;              // > 0: the update is applied only when gamma <= gate
    double *delta_x;          // out: d (zero unless applied)
    double *gamma;            // out: r^T S^-1 r (0 when S is not positive definite)
    double *pos_var_out;      // out, 3: P(12,12), P(13,13), P(14,14) after the call, or null
};

// ---- launchers (ekf_kernels.hip, ekf_linalg.hip, ekf_direct.hip): d = n descriptors in device-addressable memory, one per stream
extern "C" {
void ekf_launch_propagate(const EkfStreamDev *d, int n, hipStream_t st);
void ekf_launch_remove_clone(const EkfStreamDev *d, int n, hipStream_t st);
void ekf_launch_features(const EkfStreamDev *d, const int *work_wave, int n_wave, const int *work_small, int n_small, const int *work_big, int n_big,
                         int max_rows, int max_rows_small, int big_clones, hipStream_t st);
void ekf_launch_pair_features(const EkfStreamDev *d, int n, int max_feat, int max_tri, hipStream_t st);
void ekf_launch_posvar(const EkfStreamDev *d, int n, double *out, hipStream_t st);
void ekf_launch_posvar_upd(const EkfStreamDev *d, int n, hipStream_t st);
void ekf_launch_odom_cov(const EkfStreamDev *d, int n, double *out, hipStream_t st);      // out: 48 doubles per stream (mskf_odom_cov)
void ekf_launch_gemm(const EkfStreamDev *d, int n, int mode, int max_mn, hipStream_t st);
void ekf_launch_chol(const EkfStreamDev *d, int n, int which, int min_d, int max_d, hipStream_t st);
void ekf_launch_tsqr(const EkfStreamDev *d, int n, int min_d, int max_d, int do_cap, hipStream_t st);
void ekf_launch_trsm(const EkfStreamDev *d, int n, int max_d, hipStream_t st);
void ekf_launch_small_update(const EkfStreamDev *d, int n, int max_d, hipStream_t st);
void ekf_launch_direct_update(const EkfDirectDev *d, int n, hipStream_t st);
}

struct EkfStreamState {       // host-side bookkeeping of the device buffers of one stream
    int max_clones = 0, ld = 0, d = EKF_IMU_DIM;
    int max_rows = 0, max_feat = 0, max_obs = 0, nmax = 0;
    bool hs_async = false;    // Hs came from the stream-ordered allocator (grown during a run)
    double *pool = nullptr;   // one allocation: P, T, S, W, P_alt, act, gate_S, chi2
    double *P = nullptr, *Hs = nullptr, *rs = nullptr, *T = nullptr, *S = nullptr, *W = nullptr, *gate_S = nullptr;
    int *act = nullptr;       // ld ints: active column list of the current update
    double *chi2 = nullptr;
};
