// csrc/hip/fe_cam_models.h (the header the extended track kernel and the C ABI run) compiled for the host: a small shared library
// for tests/test_camera_models_reference.py, which compares it with the numpy restatement (tests/camera_models_reference.py).
#include <cstddef>
#include "msckf_stereo_c_amd/csrc/hip/fe_cam_models.h"

extern "C" {
// pixels (n x 2 float32) -> normalised float32 coordinates through R (9 doubles, or null for the identity path); ok[i] = in the domain
void fcm_undistort_points(int n, const double *K, int model, const double *coef, const double *R, const float *px, float *out, uint8_t *ok) {
    for (int i = 0; i < n; ++i) ok[i] = fcm_undistort_px(K, model, coef, R, px[2 * i], px[2 * i + 1], out[2 * i], out[2 * i + 1]) ? 1 : 0;
}
// rays (n x 2 float32, z = 1) -> float32 pixels
void fcm_distort_points(int n, const double *K, int model, const double *coef, const float *xy, float *out, uint8_t *ok) {
    for (int i = 0; i < n; ++i) ok[i] = fcm_distort_px(K, model, coef, xy[2 * i], xy[2 * i + 1], out[2 * i], out[2 * i + 1]) ? 1 : 0;
}
// the model functions on doubles (normalised in, normalised out), for the domain edges
int fcm_undistort_norm(int model, const double *coef, double *xy) { return fcm_undistort(model, coef, xy[0], xy[1]) ? 1 : 0; }
int fcm_distort_norm(int model, const double *coef, const double *xy, double *out) { return fcm_distort(model, coef, xy[0], xy[1], out[0], out[1]) ? 1 : 0; }
// the double-sphere ray of a normalised pixel (before the z rule): ray[3]; 0 = refused by the r2 rule
int fcm_ds_ray_norm(const double *coef, const double *xy, double *ray) { return fcm_ds_ray(coef, xy[0], xy[1], ray[0], ray[1], ray[2]) ? 1 : 0; }
int fcm_validate_model(int model, const double *coef) { return fcm_validate(model, coef); }
double fcm_det_atan(double x) { return det_atan(x); }
double fcm_det_tan(double x) { return det_tan(x); }

// sizeof(FeCamExtDev) and the offsets of its fields
int fcm_dev_layout(int *out, int capacity) {
    const int v[] = {(int)sizeof(FeCamExtDev), (int)offsetof(FeCamExtDev, model), (int)offsetof(FeCamExtDev, coef), FCM_COEFFS};
    const int n = (int)(sizeof(v) / sizeof(v[0]));
    for (int i = 0; i < n && i < capacity; ++i) out[i] = v[i];
    return n;
}
}
