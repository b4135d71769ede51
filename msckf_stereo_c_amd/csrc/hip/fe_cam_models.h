// fe_cam_models.h — the opt-in camera models of the front end ("Extended camera models"): OpenCV's rational
// radtan with up to eight coefficients, Kalibr's fov (Devernay-Faugeras ATAN) distortion and the double-sphere camera.  ONE
// source for their arithmetic: the extended instantiation of the track kernel (fe_kernels.hip, k_track4_ext), the setter of
// the C ABI and the g++-compiled CPU harness (tests/cpp/fe_cam_models_test.cpp) all run these functions.  IEEE double,
// + - * / sqrt only, compiled with -ffp-contract=off like everything else; atan / tan are the project's own det_atan /
// det_tan (libm and the device library do not round alike), which therefore live here too.
//
// A model function takes and returns NORMALISED image coordinates; fcm_undistort_px / fcm_distort_px at the end put the pixel
// step (u - cx) / fx before and xd * fx + cx after, the rotation R01 and the rounding to float32 around it exactly as
// undistort_pt / distort_pt (fe_kernels.hip) have them for the base models.  A function returns false for a point outside the
// model's domain; the two base models never refuse one.
//   radtan8  k1 k2 p1 p2 k3 k4 k5 k6 (OpenCV order).  With k3 = .. = k6 = 0 every operation below that touches them is exact
//            (numerator exactly 1, 0 * r2 + k2 exactly k2, trailing factor exactly 1.0): the bits of the base radtan.
//   fov      w, radians, 0 < w < pi.
//   ds       xi, alpha, -1 < xi <= 1, 0 <= alpha <= 1 (Usenko, Demmel, Cremers 2018), rays on the z = 1 plane.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define FCM_FN __host__ __device__ __forceinline__
#else
#define FCM_FN inline
#endif

enum { FCM_RADTAN = 0, FCM_EQUIDISTANT = 1, FCM_RADTAN8 = 2, FCM_FOV = 3, FCM_DS = 4, FCM_N_MODELS = 5 };     // == MSKF_MODEL_*
#define FCM_COEFFS 8
#define FCM_FLOOR 1e-8                       // below this radius fov's scale is its limit
#define FCM_HALF_PI 1.5707963267948966       // the double nearest pi/2: fov's domain is rd * w < this

// What the extended track kernel reads of a stream beside its FeStreamDev: element i of a second array goes with descriptor i
// of the launch.  model[c] is camera c's model, base or extended; a base model's coefficients stay in CamDev::D.
struct FeCamExtDev {
    int model[2];
    double coef[2][FCM_COEFFS];
};

// how many coefficients a model takes (0: no such model)
FCM_FN int fcm_n_coeffs(int model) {
    return model == FCM_RADTAN || model == FCM_EQUIDISTANT ? 4 : model == FCM_RADTAN8 ? 8 : model == FCM_FOV ? 1 : model == FCM_DS ? 2 : 0;
}

// The setter's check of a model's coefficients: 0 = fine, else which rule failed (1 unknown model, 2 not finite, 3 w outside
// (0, pi), 4 xi outside (-1, 1], 5 alpha outside [0, 1]).  Coefficients past the model's own must be finite too (they are kept).
FCM_FN int fcm_validate(int model, const double *c) {
    if (fcm_n_coeffs(model) == 0) return 1;
    for (int i = 0; i < FCM_COEFFS; ++i) if (!(c[i] - c[i] == 0.0)) return 2;
    if (model == FCM_FOV && !(c[0] > 0.0 && c[0] < 3.141592653589793)) return 3;
    if (model == FCM_DS && !(c[0] > -1.0 && c[0] <= 1.0)) return 4;
    if (model == FCM_DS && !(c[1] >= 0.0 && c[1] <= 1.0)) return 5;
    return 0;
}

// ------------------------------------------------------------------------------------------ det_atan / det_tan
// Deterministic atan / tan for the equidistant (fisheye) and fov camera models.  cv::fisheye::distortPoints needs atan(r),
// cv::fisheye::undistortPoints needs tan(theta); libm and the GPU math library do not round them identically, so both
// sides evaluate the SAME sequence of IEEE double operations (+ - * / only, no contraction): argument reduction to a
// small interval and an odd Taylor polynomial.  Accuracy as doubles: within 8 * 2^-53 = 8.9e-16 relative of tanl on
// (0, pi/2] and of atanl on (0, 1e300) (observed 4.5e-16 / 4.1e-16; tests/test_camera_reference.py sweeps oracle/o_math.h's
// copy); through the camera models the float32 outputs equal the rounded long-double model
// (tests/test_gpu_camera_geometry.py on the device).

// atan(x), x >= 0:  x > 1 -> pi/2 - atan(1/x);  then atan(x) = atan(c) + atan((x - c) / (1 + x c)) with the nearest
// c in {0, 1/4, 1/2, 3/4, 1} (|z| <= 1/8 -> 11 odd terms leave < 1e-21)
FCM_FN double det_atan(double x) {
    const bool inv = x > 1.0;
    if (inv) x = 1.0 / x;
    double c = 0.0, ac = 0.0;
    if (x > 0.875)      { c = 1.0;  ac = 0.78539816339744830962; }
    else if (x > 0.625) { c = 0.75; ac = 0.64350110879328438680; }
    else if (x > 0.375) { c = 0.5;  ac = 0.46364760900080611621; }
    else if (x > 0.125) { c = 0.25; ac = 0.24497866312686415417; }
    const double z = (x - c) / (1.0 + x * c);
    const double z2 = z * z;
    double p = 1.0 / 21.0;
    p = 1.0 / 19.0 - z2 * p;
    p = 1.0 / 17.0 - z2 * p;
    p = 1.0 / 15.0 - z2 * p;
    p = 1.0 / 13.0 - z2 * p;
    p = 1.0 / 11.0 - z2 * p;
    p = 1.0 / 9.0 - z2 * p;
    p = 1.0 / 7.0 - z2 * p;
    p = 1.0 / 5.0 - z2 * p;
    p = 1.0 / 3.0 - z2 * p;
    p = 1.0 - z2 * p;
    const double a = ac + z * p;
    return inv ? 1.5707963267948966192 - a : a;
}
// tan(t), 0 <= t <= pi/2:  t > pi/4 -> 1 / tan(pi/2 - t);  tan = sin / cos with Taylor series on [0, pi/4].  pi/2 is taken
// in two parts (the double nearest it, whose difference with t is exact for t >= pi/4, plus the 6.1e-17 that double lacks):
// with one part the reduced argument is 0 at the double pi/2, where undistort_pt clamps theta_d, and tan there is inf.
FCM_FN double det_tan(double t) {
    const bool inv = t > 0.78539816339744830962;
    if (inv) t = (1.5707963267948966192 - t) + 6.123233995736766e-17;
    const double t2 = t * t;
    double s = 1.0 / 121645100408832000.0;              // 1/19!
    s = 1.0 / 355687428096000.0 - t2 * s;                // 1/17!
    s = 1.0 / 1307674368000.0 - t2 * s;                  // 1/15!
    s = 1.0 / 6227020800.0 - t2 * s;                     // 1/13!
    s = 1.0 / 39916800.0 - t2 * s;                       // 1/11!
    s = 1.0 / 362880.0 - t2 * s;                         // 1/9!
    s = 1.0 / 5040.0 - t2 * s;                           // 1/7!
    s = 1.0 / 120.0 - t2 * s;                            // 1/5!
    s = 1.0 / 6.0 - t2 * s;                              // 1/3!
    s = t * (1.0 - t2 * s);
    double c = 1.0 / 6402373705728000.0;                 // 1/18!
    c = 1.0 / 20922789888000.0 - t2 * c;                 // 1/16!
    c = 1.0 / 87178291200.0 - t2 * c;                    // 1/14!
    c = 1.0 / 479001600.0 - t2 * c;                      // 1/12!
    c = 1.0 / 3628800.0 - t2 * c;                        // 1/10!
    c = 1.0 / 40320.0 - t2 * c;                          // 1/8!
    c = 1.0 / 720.0 - t2 * c;                            // 1/6!
    c = 1.0 / 24.0 - t2 * c;                             // 1/4!
    c = 0.5 - t2 * c;                                    // 1/2!
    c = 1.0 - t2 * c;
    return inv ? c / s : s / c;
}

// ------------------------------------------------------------------------------------------ radtan8
// cv::undistortPoints with eight coefficients: the five fixed-point steps of the base radtan, icdist rational
FCM_FN bool fcm_radtan8_undistort(const double *k, double &x, double &y) {
    const double k1 = k[0], k2 = k[1], p1 = k[2], p2 = k[3], k3 = k[4], k4 = k[5], k5 = k[6], k6 = k[7];
    const double x0 = x, y0 = y;
    for (int j = 0; j < 5; ++j) {
        const double r2 = x * x + y * y;
        const double icdist = (1.0 + ((k6 * r2 + k5) * r2 + k4) * r2) / (1.0 + ((k3 * r2 + k2) * r2 + k1) * r2);
        const double deltaX = 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x);
        const double deltaY = p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y;
        x = (x0 - deltaX) * icdist;
        y = (y0 - deltaY) * icdist;
    }
    return true;
}
// cv::projectPoints with eight coefficients
FCM_FN bool fcm_radtan8_distort(const double *k, double x, double y, double &xd, double &yd) {
    const double k1 = k[0], k2 = k[1], p1 = k[2], p2 = k[3], k3 = k[4], k4 = k[5], k5 = k[6], k6 = k[7];
    const double r2 = x * x + y * y, r4 = r2 * r2, r6 = r4 * r2;
    const double a1 = 2.0 * x * y, a2 = r2 + 2.0 * x * x, a3 = r2 + 2.0 * y * y;
    const double cdist = 1.0 + k1 * r2 + k2 * r4 + k3 * r6;
    const double icdist2 = 1.0 / (1.0 + k4 * r2 + k5 * r4 + k6 * r6);
    xd = x * cdist * icdist2 + p1 * a1 + p2 * a2;
    yd = y * cdist * icdist2 + p1 * a3 + p2 * a1;
    return true;
}

// ------------------------------------------------------------------------------------------ fov
// rd = sqrt(xd^2 + yd^2); ru = tan(rd w) / (2 tan(w / 2)); scale ru / rd, below the floor its limit w / (2 tan(w / 2)).
// Outside the domain when rd w >= pi/2 (the ray would lie in or behind the image plane).
FCM_FN bool fcm_fov_undistort(const double *k, double &x, double &y) {
    const double w = k[0];
    const double two_tw = 2.0 * det_tan(w * 0.5);
    const double rd = sqrt(x * x + y * y);
    const double a = rd * w;
    if (!(a < FCM_HALF_PI)) return false;
    double scale = w / two_tw;
    if (!(rd < FCM_FLOOR)) {
        const double ru = det_tan(a) / two_tw;
        scale = ru / rd;
    }
    x = x * scale; y = y * scale;
    return true;
}
// ru = sqrt(x^2 + y^2); rd = atan(2 ru tan(w / 2)) / w; scale rd / ru, below the floor its limit 2 tan(w / 2) / w
FCM_FN bool fcm_fov_distort(const double *k, double x, double y, double &xd, double &yd) {
    const double w = k[0];
    const double two_tw = 2.0 * det_tan(w * 0.5);
    const double ru = sqrt(x * x + y * y);
    double scale = two_tw / w;
    if (!(ru < FCM_FLOOR)) {
        const double rd = det_atan(two_tw * ru) / w;
        scale = rd / ru;
    }
    xd = x * scale; yd = y * scale;
    return true;
}

// ------------------------------------------------------------------------------------------ ds
// Unprojection of the paper, then the ray onto z = 1.  Outside the domain: alpha > 0.5 and r2 > 1 / (2 alpha - 1); ray z <= 0
// (or no number).  1 - (2 alpha - 1) r2 is clamped at 0: at r2 = the rounded 1 / (2 alpha - 1) it may round below it.
// (the paper's unprojection itself: the ray through the normalised pixel (mx, my), not yet scaled; false = the first rule)
FCM_FN bool fcm_ds_ray(const double *k, double mx, double my, double &rx, double &ry, double &rz) {
    const double xi = k[0], alpha = k[1];
    const double r2 = mx * mx + my * my;
    const double b = 2.0 * alpha - 1.0;
    if (alpha > 0.5 && r2 > 1.0 / b) return false;
    double sa = 1.0 - b * r2;
    if (sa < 0.0) sa = 0.0;
    const double s = sqrt(sa);
    const double mz = (1.0 - alpha * alpha * r2) / (alpha * s + 1.0 - alpha);
    const double mz2 = mz * mz;
    const double t = (mz * xi + sqrt(mz2 + (1.0 - xi * xi) * r2)) / (mz2 + r2);
    rx = t * mx; ry = t * my; rz = t * mz - xi;
    return true;
}
FCM_FN bool fcm_ds_undistort(const double *k, double &x, double &y) {
    double rx, ry, rz;
    if (!fcm_ds_ray(k, x, y, rx, ry, rz)) return false;
    if (!(rz > 0.0)) return false;
    x = rx / rz; y = ry / rz;
    return true;
}
// Projection of the ray (x, y, 1).  Outside the domain when 1 > -w2 d1 fails (w1 = alpha / (1 - alpha) for alpha <= 0.5, else
// (1 - alpha) / alpha; w2 = (w1 + xi) / sqrt(2 w1 xi + xi^2 + 1)) or the denominator is not positive.
FCM_FN bool fcm_ds_distort(const double *k, double x, double y, double &xd, double &yd) {
    const double xi = k[0], alpha = k[1];
    const double r2 = x * x + y * y;
    const double d1 = sqrt(r2 + 1.0);
    const double kk = xi * d1 + 1.0;
    const double d2 = sqrt(r2 + kk * kk);
    const double den = alpha * d2 + (1.0 - alpha) * kk;
    const double w1 = alpha > 0.5 ? (1.0 - alpha) / alpha : alpha / (1.0 - alpha);
    const double w2 = (w1 + xi) / sqrt(2.0 * w1 * xi + xi * xi + 1.0);
    if (!(1.0 > -w2 * d1) || !(den > 0.0)) return false;
    xd = x / den; yd = y / den;
    return true;
}

// ------------------------------------------------------------------------------------------ by model
// the extended models only (model >= FCM_RADTAN8); k = the model's coefficients
FCM_FN bool fcm_undistort(int model, const double *k, double &x, double &y) {
    if (model == FCM_RADTAN8) return fcm_radtan8_undistort(k, x, y);
    if (model == FCM_FOV) return fcm_fov_undistort(k, x, y);
    return fcm_ds_undistort(k, x, y);
}
FCM_FN bool fcm_distort(int model, const double *k, double x, double y, double &xd, double &yd) {
    if (model == FCM_RADTAN8) return fcm_radtan8_distort(k, x, y, xd, yd);
    if (model == FCM_FOV) return fcm_fov_distort(k, x, y, xd, yd);
    return fcm_ds_distort(k, x, y, xd, yd);
}

// Pixel -> normalised (rotated by R, rows X Y W, unless R is null) float32 coordinates; K = fx fy cx cy.  Outside the domain: false
// and (0, 0).
FCM_FN bool fcm_undistort_px(const double *K, int model, const double *k, const double *R, float u, float v, float &xo, float &yo) {
    const double fx = K[0], fy = K[1], cx = K[2], cy = K[3];
    double x = ((double)u - cx) / fx, y = ((double)v - cy) / fy;
    xo = 0.f; yo = 0.f;
    if (!fcm_undistort(model, k, x, y)) return false;
    if (R) {
        const double X = R[0] * x + R[1] * y + R[2];
        const double Y = R[3] * x + R[4] * y + R[5];
        const double Wd = R[6] * x + R[7] * y + R[8];
        x = X / Wd; y = Y / Wd;
    } else {
        x = x / 1.0; y = y / 1.0;
    }
    xo = (float)(x * 1.0 + 0.0);
    yo = (float)(y * 1.0 + 0.0);
    return true;
}
// The ray (xf, yf, 1) -> float32 pixel.  Outside the domain: false and (0, 0).
FCM_FN bool fcm_distort_px(const double *K, int model, const double *k, float xf, float yf, float &uo, float &vo) {
    const double fx = K[0], fy = K[1], cx = K[2], cy = K[3];
    double xd, yd;
    uo = 0.f; vo = 0.f;
    if (!fcm_distort(model, k, (double)xf, (double)yf, xd, yd)) return false;
    uo = (float)(xd * fx + cx);
    vo = (float)(yd * fy + cy);
    return true;
}
