"""ctypes mirrors of include/mskf_types.h (POD only; no behaviour)."""
import ctypes as C

import numpy as np


class Calib(C.Structure):
    _fields_ = [
        ("width", C.c_int32), ("height", C.c_int32),
        ("cam0_intrinsics", C.c_double * 4), ("cam0_distortion", C.c_double * 4),
        ("cam0_model", C.c_int32), ("cam1_model", C.c_int32),
        ("cam1_intrinsics", C.c_double * 4), ("cam1_distortion", C.c_double * 4),
        ("T_cam0_imu", C.c_double * 16), ("T_cam1_cam0", C.c_double * 16), ("T_imu_body", C.c_double * 16),
    ]


class FeCfg(C.Structure):
    _fields_ = [
        ("grid_row", C.c_int32), ("grid_col", C.c_int32),
        ("grid_min_feature_num", C.c_int32), ("grid_max_feature_num", C.c_int32),
        ("pyramid_levels", C.c_int32), ("patch_size", C.c_int32),
        ("fast_threshold", C.c_int32), ("max_iteration", C.c_int32),
        ("track_precision", C.c_double), ("ransac_threshold", C.c_double), ("stereo_threshold", C.c_double),
        ("det_rows", C.c_int32), ("det_cols", C.c_int32),
        ("compat_flags", C.c_int32), ("_pad", C.c_int32),
    ]


class EkfCfg(C.Structure):
    _fields_ = [
        ("frame_rate", C.c_double),
        ("max_cam_state_size", C.c_int32), ("chi2_mode", C.c_int32),
        ("position_std_threshold", C.c_double), ("rotation_threshold", C.c_double),
        ("translation_threshold", C.c_double), ("tracking_rate_threshold", C.c_double),
        ("feature_translation_threshold", C.c_double),
        ("noise_gyro", C.c_double), ("noise_acc", C.c_double), ("noise_gyro_bias", C.c_double),
        ("noise_acc_bias", C.c_double), ("noise_feature", C.c_double),
        ("init_velocity", C.c_double * 3),
        ("cov_velocity", C.c_double), ("cov_gyro_bias", C.c_double), ("cov_acc_bias", C.c_double),
        ("cov_ext_rot", C.c_double), ("cov_ext_trans", C.c_double),
        ("max_stack_rows", C.c_int32), ("compression_mode", C.c_int32),
    ]


class ImuSample(C.Structure):
    _fields_ = [("time_stamp", C.c_double), ("angular_velocity", C.c_double * 3),
                ("linear_acceleration", C.c_double * 3)]


class ImuStep(C.Structure):
    """mskf_imu_step (include/mskf_hip.h): what the covariance part of processModel needs for one IMU sample."""
    _fields_ = [("dt", C.c_double), ("gyro", C.c_double * 3), ("acc", C.c_double * 3), ("R_t", C.c_double * 9),
                ("Phi00", C.c_double * 9), ("u", C.c_double * 3), ("s", C.c_double * 3), ("w1", C.c_double * 3),
                ("w2", C.c_double * 3)]


assert C.sizeof(ImuStep) == 37 * 8


class TrackingInfo(C.Structure):
    _fields_ = [("time_stamp", C.c_double), ("before_tracking", C.c_int32), ("after_tracking", C.c_int32),
                ("after_matching", C.c_int32), ("after_ransac", C.c_int32)]


class OdomCov(C.Structure):
    """mskf_odom_cov (include/mskf_types.h): covariance half of the published odometry."""
    _fields_ = [("pose", C.c_double * 36), ("twist", C.c_double * 9), ("pos_var", C.c_double * 3)]


class EkfDirectArgs(C.Structure):
    """mskf_ekf_direct_args (include/mskf_hip.h): a direct measurement update of up to DIRECT_MAX_ROWS rows on the IMU block."""
    _fields_ = [("m", C.c_int32), ("status", C.c_int32), ("H", C.c_void_p), ("r", C.c_void_p), ("R", C.c_void_p), ("gate", C.c_double),
                ("delta_x", C.c_void_p), ("gamma", C.c_double), ("pos_var_out", C.c_void_p)]


assert C.sizeof(EkfDirectArgs) == 64
DIRECT_MAX_ROWS = 6          # MSKF_DIRECT_MAX_ROWS (csrc/hip/ekf_limits.h)


class FeEqualize(C.Structure):
    """mskf_fe_equalize (include/mskf_hip.h): opt-in equalisation of the pushed images; mode 0 off, 1 global, 2 CLAHE."""
    _fields_ = [("mode", C.c_int32), ("tiles_x", C.c_int32), ("tiles_y", C.c_int32), ("_pad", C.c_int32), ("clip_limit", C.c_double)]


assert C.sizeof(FeEqualize) == 24
EQUALIZE_MODES = {"off": 0, "hist": 1, "clahe": 2}


class FeInputFormat(C.Structure):
    """mskf_fe_input_format (include/mskf_hip.h): the pixel format of the pushed images; shift goes with gray16 only."""
    _fields_ = [("format", C.c_int32), ("shift", C.c_int32)]


assert C.sizeof(FeInputFormat) == 8
# MSKF_PIX_*: a Bayer name spells the 2 x 2 tile at the image's top-left corner in reading order (not OpenCV's naming)
INPUT_FORMATS = {"gray8": 0, "gray16": 1, "rgb8": 2, "bgr8": 3, "rgba8": 4, "bgra8": 5,
                 "bayer_rggb8": 6, "bayer_grbg8": 7, "bayer_gbrg8": 8, "bayer_bggr8": 9}
INPUT_FORMAT_BPP = [1, 2, 3, 3, 4, 4, 1, 1, 1, 1]


class FeMask(C.Structure):
    """mskf_fe_mask (include/mskf_hip.h): per-camera image masks, a pixel != 0 is usable; a null plane = that camera is not masked."""
    _fields_ = [("cam0", C.c_void_p), ("cam1", C.c_void_p), ("width", C.c_int32), ("height", C.c_int32), ("pitch", C.c_int32), ("margin", C.c_int32)]


assert C.sizeof(FeMask) == 32
MASK_MAX_MARGIN = 64         # FM_MAX_MARGIN (csrc/hip/fe_mask.h)


class FePatchCheck(C.Structure):
    """mskf_fe_patch_check (include/mskf_hip.h): the ZNCC patch check of temporal tracks (mode bit 1) and stereo matches (bit 2)."""
    _fields_ = [("mode", C.c_int32), ("half", C.c_int32), ("min_zncc_temporal", C.c_float), ("min_zncc_stereo", C.c_float)]


assert C.sizeof(FePatchCheck) == 16
PATCH_CHECK_MODES = {"off": 0, "temporal": 1, "stereo": 2, "both": 3}


class FeFbCheck(C.Structure):
    """mskf_fe_fb_check (include/mskf_hip.h): the forward-backward check of temporal tracks (mode bit 1) and stereo matches (bit 2)."""
    _fields_ = [("mode", C.c_int32), ("max_error_temporal", C.c_float), ("max_error_stereo", C.c_float)]


assert C.sizeof(FeFbCheck) == 12
FB_CHECK_MODES = {"off": 0, "temporal": 1, "stereo": 2, "both": 3}
FB_MAX_ERROR = 64.0          # FB_MAX_ERROR (csrc/hip/fe_fb.h)


class FeCameraModel(C.Structure):
    """mskf_fe_camera_model (include/mskf_hip.h): one camera's model and its coefficients (unused ones 0)."""
    _fields_ = [("cam", C.c_int32), ("model", C.c_int32), ("coeffs", C.c_double * 8)]


CAMERA_MODELS = {"radtan": 0, "equidistant": 1, "radtan8": 2, "fov": 3, "ds": 4}      # MSKF_MODEL_*
CAMERA_MODEL_COEFFS = {0: (4,), 1: (4,), 2: (5, 8), 3: (1,), 4: (2,)}                  # how many coefficients a model may be given


def camera_model_cfg(cam, model, coeffs):
    """FeCameraModel of (cam, model name or number, coefficients): the coefficients are padded with zeros to eight (radtan8 takes
    OpenCV's five or eight).  Raises ValueError on an unknown model name or a wrong count; the library checks the values."""
    if isinstance(model, str) and model not in CAMERA_MODELS:
        raise ValueError("unknown camera model %r (one of %s)" % (model, ", ".join(CAMERA_MODELS)))
    m = int(CAMERA_MODELS.get(model, model))
    k = [float(v) for v in coeffs]
    if m in CAMERA_MODEL_COEFFS and len(k) not in CAMERA_MODEL_COEFFS[m]:
        raise ValueError("camera model %r takes %s coefficients, not %d" % (model, " or ".join(map(str, CAMERA_MODEL_COEFFS[m])), len(k)))
    if len(k) > 8:
        raise ValueError("a camera model takes at most 8 coefficients")
    return FeCameraModel(int(cam), m, (C.c_double * 8)(*(k + [0.0] * (8 - len(k)))))


class FeDescribeArgs(C.Structure):
    """mskf_fe_describe_args (include/mskf_hip.h): n points of the image of `role` in, 32 n descriptor bytes and n validity bytes out."""
    _fields_ = [("role", C.c_int32), ("n", C.c_int32), ("pts", C.c_void_p), ("desc", C.c_void_p), ("valid", C.c_void_p)]


assert C.sizeof(FeDescribeArgs) == 32
DESCRIPTOR_BYTES = 32        # FB_BYTES (csrc/hip/fe_brief.h)


class FeMatchArgs(C.Structure):
    """mskf_fe_match_args (include/mskf_hip.h): nq query against nt train descriptors with their optional validity arrays in, nq
    mskf_match records and their count of accepted ones out."""
    _fields_ = [("nq", C.c_int32), ("nt", C.c_int32), ("query", C.c_void_p), ("query_valid", C.c_void_p), ("train", C.c_void_p), ("train_valid", C.c_void_p),
                ("max_distance", C.c_int32), ("ratio", C.c_float), ("cross_check", C.c_int32), ("matches", C.c_void_p), ("n_matches", C.c_int32)]


assert C.sizeof(FeMatchArgs) == 72
MATCH = np.dtype([("idx", "<i4"), ("nearest", "<i4"), ("dist", "<u2"), ("second", "<u2")])       # mskf_match
assert MATCH.itemsize == 12
MATCH_MAX_N = 65535          # FM_MAX_N (csrc/hip/fe_match.h)
MATCH_NONE = 0xFFFF          # FM_NONE: dist / second without a neighbour


class FeVerifyArgs(C.Structure):
    """mskf_fe_verify_args (include/mskf_hip.h): n pairs of stereo observations, the camera pair, the hypothesis count, seed and
    thresholds in; the counts, the winning hypothesis, its inlier bytes, the refined pose, its information matrix and rms out."""
    _fields_ = [("n", C.c_int32), ("n_hypotheses", C.c_int32), ("query_obs", C.c_void_p), ("train_obs", C.c_void_p), ("usable", C.c_void_p),
                ("T_cam1_cam0", C.c_double * 16), ("seed", C.c_uint64), ("max_error", C.c_double), ("min_depth", C.c_double), ("max_depth", C.c_double),
                ("inlier", C.c_void_p), ("n_usable", C.c_int32), ("n_inliers", C.c_int32), ("best", C.c_int32), ("status", C.c_int32),
                ("R", C.c_double * 9), ("t", C.c_double * 3), ("info", C.c_double * 36), ("rms", C.c_double)]


assert C.sizeof(FeVerifyArgs) == 608
VERIFY_MAX_N = 4096          # FV_MAX_N (csrc/hip/fe_verify.h)
VERIFY_MAX_K = 1024          # FV_MAX_K


def raw_raster(img, fmt):
    """An image in format number fmt as the contiguous array a push takes: (h, w) uint16 for gray16 (native byte order, which the
    device reads as little-endian), (h, w, 3 | 4) uint8 for the colour formats, (h, w) uint8 otherwise.  A wrong shape or a
    dtype that would have to be narrowed raises."""
    img = np.asarray(img)
    bpp = INPUT_FORMAT_BPP[fmt]
    if fmt == 1:
        if img.dtype != np.uint16 or img.ndim != 2:
            raise ValueError("gray16 takes (h, w) uint16 images, not %s %s" % (img.shape, img.dtype))
        return np.ascontiguousarray(img.astype("<u2", copy=False))
    if bpp > 1 and (img.ndim != 3 or img.shape[2] != bpp or img.dtype != np.uint8):
        raise ValueError("this colour format takes (h, w, %d) uint8 images, not %s %s" % (bpp, img.shape, img.dtype))
    if bpp == 1 and fmt != 0 and (img.ndim != 2 or img.dtype != np.uint8):
        raise ValueError("a Bayer format takes (h, w) uint8 images, not %s %s" % (img.shape, img.dtype))
    return np.ascontiguousarray(img, dtype=np.uint8)


# numpy dtypes of the array records
POINT2F = np.dtype([("x", "<f4"), ("y", "<f4")])
CORNER = np.dtype([("x", "<f4"), ("y", "<f4"), ("score", "<i4"), ("cell", "<i4")])
FEATURE_MEAS = np.dtype([("id", "<u4"), ("_pad", "<u4"), ("u0", "<f8"), ("v0", "<f8"), ("u1", "<f8"), ("v1", "<f8")])
POSE = np.dtype([("t", "<f8"), ("p", "<f8", 3), ("q", "<f8", 4)])
ODOM_COV = np.dtype([("pose", "<f8", (6, 6)), ("twist", "<f8", (3, 3)), ("pos_var", "<f8", 3)])
assert ODOM_COV.itemsize == C.sizeof(OdomCov) == 384
IMU_STEP = np.dtype([(name, "<f8", C.sizeof(ty) // 8) if C.sizeof(ty) > 8 else (name, "<f8") for name, ty in ImuStep._fields_])
assert IMU_STEP.itemsize == C.sizeof(ImuStep)

COMPAT_REFERENCE = 15     # Q1 | Q2 | Q4 | Q5 (include/mskf_types.h)


def default_fe_cfg(grid_row=4, grid_col=5, grid_min=3, grid_max=4, compat=COMPAT_REFERENCE):
    """config/app_imgproc.yaml values of the reference + CornerDetector(30, 47, thr) (image_processor.cpp:132)."""
    c = FeCfg()
    c.grid_row, c.grid_col, c.grid_min_feature_num, c.grid_max_feature_num = grid_row, grid_col, grid_min, grid_max
    c.pyramid_levels, c.patch_size, c.fast_threshold, c.max_iteration = 3, 15, 10, 30
    c.track_precision, c.ransac_threshold, c.stereo_threshold = 0.01, 3.0, 5.0
    c.det_rows, c.det_cols = 30, 47
    c.compat_flags = compat
    return c


def default_ekf_cfg(max_cam_state_size=20, compression_mode=3):
    """config/app_msckfvio.yaml values of the reference.  compression_mode: 3 (default) the reference's own rule - Householder QR
    when the stack has more rows than columns, nothing otherwise (msckf_vio.cpp:795-821) -, 0 auto (Gram + regularised Cholesky,
    Householder where the device asks for it), 1 Gram + Cholesky only, 2 Householder TSQR always."""
    c = EkfCfg()
    c.frame_rate = 20.0
    c.max_cam_state_size = max_cam_state_size
    c.chi2_mode = 0
    c.position_std_threshold, c.rotation_threshold = 8.0, 0.2618
    c.translation_threshold, c.tracking_rate_threshold = 0.4, 0.5
    c.feature_translation_threshold = -1.0
    c.noise_gyro, c.noise_acc, c.noise_gyro_bias, c.noise_acc_bias, c.noise_feature = 0.005, 0.05, 0.001, 0.01, 0.035
    c.init_velocity[:] = [0.0, 0.0, 0.0]
    c.cov_velocity, c.cov_gyro_bias, c.cov_acc_bias = 0.25, 0.01, 0.01
    c.cov_ext_rot, c.cov_ext_trans = 3.0462e-4, 2.5e-5
    c.max_stack_rows = 1500
    c.compression_mode = compression_mode
    return c


# synth::RenderImg (csrc/synth/synth.h): what one image of a synthetic sequence is rendered from (input generator, host and device)
RENDER_IMG = np.dtype([("R_wc", "<f8", 9), ("o", "<f8", 3), ("pixel_sigma", "<f8"), ("seed", "<u4"), ("k2c", "<i4"), ("cam", "<i4"), ("pad", "<i4")])
