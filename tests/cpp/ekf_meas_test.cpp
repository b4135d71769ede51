// Host harness of csrc/hip/ekf_meas.h for tests/test_ekf_meas.py: the kernels' measurementJacobian source, compiled by the
// host compiler, on one observation.  `mutate` switches in one deliberate mistake (the test shows that its bar has teeth):
//   1: the observability projection is dropped (H_x = A);  2: u1 is formed with p instead of p_null.
#include <cstring>
#include "msckf_stereo_c_amd/csrc/hip/ekf_meas.h"

extern "C" void ekf_meas_run(const double *R_c0_c1, const double *t_c0_c1, const double *clone14, const double *pos, const double *z,
                             const double *gravity, int mutate, double *H_x /* 4 x 6 */, double *H_f /* 4 x 3 */, double *r /* 4 */) {
    mskf_clone_state cam;
    static_assert(sizeof(cam) == 14 * sizeof(double), "q p q_null p_null");
    std::memcpy(&cam, clone14, sizeof(cam));
    if (mutate == 2) std::memcpy(cam.p_null, cam.p, sizeof(cam.p));
    double R_w_c0[9], R_w_c1[9], t_c1_w[3], Rn[9], H[4][6];
    ekf::cam_pose(cam, R_c0_c1, t_c0_c1, R_w_c0, R_w_c1, t_c1_w, Rn);
    ekf::meas_jacobian(cam, R_w_c0, R_w_c1, t_c1_w, Rn, R_c0_c1, pos, gravity, z, H, r);
    if (mutate == 1) {
        double p_c0[3], p_c1[3];
        ekf::meas_cam_points(R_w_c0, R_w_c1, cam.p, t_c1_w, pos, p_c0, p_c1);
        ekf::meas_unprojected(R_w_c0, R_w_c1, R_c0_c1, p_c0, p_c1, H);
    }
    std::memcpy(H_x, H, sizeof(H));
    for (int i = 0; i < 4; ++i) for (int c = 0; c < 3; ++c) H_f[3 * i + c] = -H[i][3 + c];
}
