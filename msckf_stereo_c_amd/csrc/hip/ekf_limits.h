// ekf_limits.h — the numbers of the measurement update that more than one party must know: the limits a stream is routed and
// its matrices are factored by, the compression modes and their predicates, and the record the kernels hand each other and the
// host (rows_out).  Plain C++ (no HIP runtime): ekf_device.h includes it for the host and the kernels, and
// tests/cpp/ekf_limits_test.cpp compiles it with g++ alone to hold tests/update_cases.py against it.
#pragma once

#if defined(__HIPCC__)
#define EKF_HD __host__ __device__ __forceinline__
#else
#define EKF_HD inline
#endif

#define EKF_IMU_DIM 21

// ---- kernel limits the host routes by
#define MAX_CLONES_DEV 64         // largest clone window (mskf_ekf_cfg.max_cam_state_size): 4*64 = 256 block rows max per feature
#define FEAT_WAVE_CLONES 4        // wave-per-feature class of the feature kernel: Jacobian observations per feature at most
#define FEAT_SMALL_CLONES 16      // one-wavefront class: max(observations, triangulation clones) at most; above it the big class
#define TRI_SMALL_CLONES 32       // the wave-per-feature variant triangulates over at most this many clones
#define SU_MAX_NA 24              // k_ekf_small_update: active columns at most (four clones)
#define MSKF_DIRECT_MAX_ROWS 6    // k_ekf_direct_update: rows of a caller-supplied measurement at most (mskf_ekf_direct_args.m)
static_assert(FEAT_WAVE_CLONES <= FEAT_SMALL_CLONES && FEAT_SMALL_CLONES <= TRI_SMALL_CLONES && TRI_SMALL_CLONES <= MAX_CLONES_DEV, "size classes nest");
static_assert(MAX_CLONES_DEV <= 64, "clone sets are 64-bit masks (EkfFeatDev::colmask, rowmask)");

// ---- limits the dense kernels of the update branch on (ekf_linalg.hip)
#define EKF_GEMM_TILE 32          // k_ekf_gemm: output tile edge (GT there)
#define SU_CH 128                 // k_ekf_small_update: stacked rows per Gram chunk and per TSQR block of a wavefront
#define CHOL_LDS_MAX_ROWS 181     // k_ekf_chol_lds: active rows incl. the extra Q^T r row
#define CHOL_PAN_RS 192           // k_ekf_chol_lds: row stride of the k-major panel (rows padded to a multiple of 16)
#define TQ_THREADS 512            // k_ekf_tsqr: threads of a workgroup, four per column of a slab
#define TS_RB 16                  // k_ekf_trsm: rows of L per staged block
#define TS_LPF 14                 // k_ekf_trsm: registers of the L prefetch, 16 columns each: ceil((max d + 16) / 16) for d <= 208
// Gram + regularised Cholesky adds a prior lambda I to the stacked information H^T H / sigma^2: the posterior covariance
// moves by about lambda max(P_aa) / sigma^2 relative.  Above this limit the compression runs as Householder TSQR instead, which has no such term.
#define QR_BIAS_LIMIT 1e-6
// Which kernel handles a stream is a property of the stream's own dimension d, whatever else is in the batch.
// factorisation: 0 = k_ekf_chol_lds (the factor fits LDS), 1 = k_ekf_chol (global memory)
EKF_HD int chol_class(int d) { return d - EKF_IMU_DIM + 1 <= CHOL_LDS_MAX_ROWS ? 0 : 1; }
// k_ekf_tsqr: 0 = <32, 2, 2> (up to 2 * TQ_THREADS / 4 columns incl. the residual), 1 = <16, 4, 2>
EKF_HD int tsqr_class(int d) { return d - EKF_IMU_DIM + 1 <= 2 * (TQ_THREADS / 4) ? 0 : 1; }
// k_ekf_trsm: the row blocks of an n-row L fit the register prefetch (else they are staged directly)
EKF_HD bool trsm_l_fits(int n) { return n + TS_RB <= 16 * TS_LPF; }

// ---- qr_mode (mskf_ekf_cfg.compression_mode): auto, Gram only, Householder always, the reference literally
// (msckf_vio.cpp:795-821): Householder QR when the stack has more rows than columns, nothing otherwise.
enum { EKF_QR_AUTO = 0, EKF_QR_GRAM = 1, EKF_QR_HOUSEHOLDER = 2, EKF_QR_REFERENCE = 3 };
EKF_HD bool ekf_mode_direct(int qr_mode, int stacked, int na) { return (qr_mode == EKF_QR_AUTO || qr_mode == EKF_QR_REFERENCE) && stacked <= na; }
EKF_HD bool ekf_mode_householder(int qr_mode) { return qr_mode == EKF_QR_HOUSEHOLDER || qr_mode == EKF_QR_REFERENCE; }
// Is the compression (re-)done as Householder TSQR?  Always in the Householder modes; in auto mode when there is no Gram factor
// to use (none was formed, or the stack has no more rows than columns and H^T H is singular by construction) or when the
// factorisation raised the bias flag.  (The general route never asks with st <= na in auto mode: ekf_mode_direct took the stream.)
EKF_HD bool ekf_mode_redo_householder(int qr_mode, bool gram_factor, bool bias) { return ekf_mode_householder(qr_mode) || (qr_mode == EKF_QR_AUTO && (!gram_factor || bias)); }

// ---- EkfStreamDev::rows_out: what the first dense kernel of an update (ekf_cap.h) and the factorisation write down for the
// kernels that follow and for the host
enum {
    EKF_ROWS_STACKED = 0,         // stacked rows (0: no update applied)
    EKF_ROWS_END = 1,             // last stacked row + 1: the K range of the Gram pass and the TSQR
    EKF_ROWS_NA = 2,              // active columns
    EKF_ROWS_DIAG = 3,            // compression diagnostics, EKF_DIAG_* below
    EKF_ROWS_NK = 4,              // rows of the compressed measurement = dimension of S: na, or the stacked rows without compression
    EKF_ROWS_COUNT = 5
};
enum {
    EKF_DIAG_HOUSEHOLDER = 1,     // the compression ran as Householder TSQR
    EKF_DIAG_BIAS = 2,            // the lambda prior of the Gram path would bias P by more than QR_BIAS_LIMIT (auto mode then re-does the compression as TSQR)
    EKF_DIAG_DIRECT = 4,          // no compression (stacked rows <= active columns): the stacked rows themselves are the measurement
    EKF_DIAG_REFUSED = 0x80,      // k_ekf_tsqr: more columns than the instantiation holds (the launcher picks it from the window: cannot happen)
    EKF_DIAG_TINY_SHIFT = 8       // bits 8..: pivots of the Gram factor below 100 lambda (reported only)
};
EKF_HD int ekf_diag_encode(int tiny_pivots, bool bias) { return (tiny_pivots << EKF_DIAG_TINY_SHIFT) | (bias ? EKF_DIAG_BIAS : 0); }
// mskf_ekf_update_args.diag_out: [0] = 0 Gram factor, 1 Householder, 2 uncompressed; [1] = the tiny-pivot count
EKF_HD void ekf_diag_decode(int word, int *used_qr, int *tiny_pivots) {
    *used_qr = (word & EKF_DIAG_DIRECT) ? 2 : (word & EKF_DIAG_HOUSEHOLDER);
    *tiny_pivots = word >> EKF_DIAG_TINY_SHIFT;
}
