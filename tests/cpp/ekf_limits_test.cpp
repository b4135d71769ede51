// ekf_limits_test.cpp — prints what csrc/hip/ekf_limits.h states, one "name value" per line, for tests/test_update_limits.py
// (g++ alone: no HIP, no library): the limits the dense update kernels branch on, the class functions over every window, the
// Householder re-do predicate over all of its inputs, and the decode of a few diagnostics words.
#include <cstdio>
#include "msckf_stereo_c_amd/csrc/hip/ekf_limits.h"

int main() {
#define SHOW(name) std::printf(#name " %.17g\n", (double)(name))
    SHOW(EKF_IMU_DIM); SHOW(SU_MAX_NA); SHOW(SU_CH); SHOW(CHOL_LDS_MAX_ROWS); SHOW(CHOL_PAN_RS); SHOW(TQ_THREADS);
    SHOW(TS_RB); SHOW(TS_LPF); SHOW(EKF_GEMM_TILE); SHOW(QR_BIAS_LIMIT); SHOW(EKF_ROWS_COUNT);
    for (int w = 4; w <= 64; ++w) std::printf("class %d %d %d\n", w, chol_class(EKF_IMU_DIM + 6 * w), tsqr_class(EKF_IMU_DIM + 6 * w));
    for (int n = 1; n <= 6 * 64; ++n) std::printf("l_fits %d %d\n", n, (int)trsm_l_fits(n));
    for (int mode = 0; mode <= 3; ++mode)
        for (int gram = 0; gram <= 1; ++gram)
            for (int bias = 0; bias <= 1; ++bias) std::printf("redo %d %d %d %d\n", mode, gram, bias, (int)ekf_mode_redo_householder(mode, gram != 0, bias != 0));
    for (int mode = 0; mode <= 3; ++mode)
        for (int st = 23; st <= 25; ++st) std::printf("direct %d %d %d\n", mode, st, (int)ekf_mode_direct(mode, st, 24));
    const int words[] = {0, EKF_DIAG_HOUSEHOLDER, EKF_DIAG_DIRECT, EKF_DIAG_BIAS, EKF_DIAG_BIAS | EKF_DIAG_HOUSEHOLDER, ekf_diag_encode(3, false),
                         ekf_diag_encode(7, true) | EKF_DIAG_HOUSEHOLDER, ekf_diag_encode(300, true)};
    for (int w : words) {
        int used_qr, tiny;
        ekf_diag_decode(w, &used_qr, &tiny);
        std::printf("decode %d %d %d %d\n", w, used_qr, tiny, (w & EKF_DIAG_BIAS) ? 1 : 0);
    }
    return 0;
}
