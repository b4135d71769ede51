"""Plain long-double restatement of the per-point camera geometry of k_track4, for the kernel tests.

Written from the model definitions and from the procedure the comments of fe_kernels.hip name (cv::undistortPoints,
cv::fisheye::undistortPoints / distortPoints, cg::project_points, stereoMatch of image_processor.cpp), not from the device
code or the CPU oracle; tan and atan are the long-double library functions, not the project's polynomials.

  * pinhole: x = (u - cx) / fx, y = (v - cy) / fy; u = fx xd + cx, v = fy yd + cy.
  * radtan (k1, k2, p1, p2), distort: r2 = x^2 + y^2, xd = x (1 + k1 r2 + k2 r2^2) + 2 p1 x y + p2 (r2 + 2 x^2),
    yd = y (1 + k1 r2 + k2 r2^2) + p1 (r2 + 2 y^2) + 2 p2 x y.  Undistort: EXACTLY five fixed-point steps
    (x, y) <- ((x0, y0) - tangential(x, y)) / (1 + (k2 r2 + k1) r2) from (x0, y0): the published procedure, not the exact
    inverse (tests/test_camera_reference.py states what it leaves).
  * equidistant (Kannala-Brandt k1..k4), distort: r = |(x, y)|, theta = atan(r), theta_d = theta (1 + k1 theta^2 +
    k2 theta^4 + k3 theta^6 + k4 theta^8), (xd, yd) = (x, y) theta_d / r (r <= 1e-8: scale 1).  Undistort: theta_d =
    |(x, y)| clamped to pi/2 (the double nearest pi/2, as the published procedure has it); theta_d <= 1e-8 gives (0, 0);
    else Newton on theta from theta_d, at most 10 steps, stop after a step with |fix| < 1e-8; (x, y) tan(theta) / theta_d.
  * then the rotation R (rows X, Y, W) and the division by W.
  * stereo guess: distort(cam1, float32(undistort(cam0, R_cam0_cam1, p))); the rounding to float32 between the halves is
    part of the contract (points are float on both sides of it).
  * extrinsics as mskf_stream_create states them from T_cam0_imu / T_cam1_cam0; epipolar error |p1 . E p0| / |(E p0)_xy|.

Everything is np.longdouble.  `mutate` switches in one deliberate mistake at a time; tests/test_camera_reference.py shows
that each of them moves a well-conditioned point by 4 float32 ulps or more.
"""
import numpy as np

LD = np.longdouble
HAVE_LONG_DOUBLE = bool(np.finfo(np.longdouble).eps < 1e-18)
NEED_LONG_DOUBLE = "np.longdouble is not wider than double on this platform (eps %.1e)" % float(np.finfo(np.longdouble).eps)

RADTAN, EQUIDISTANT = 0, 1
HALF_PI_CLAMP = LD(1.5707963267948966)          # the clamp of the published procedure is the double constant
HALF_PI = LD(2) * np.arctan(LD(1))               # pi/2 to long double, for the conditioning rule
FLOOR = LD(1e-8)                                 # the floor and the stop rule likewise: the double 1e-8, widened
NEWTON_STOP = LD(1e-8)
ATAN_BOUNDS = (0.125, 0.375, 0.625, 0.875)

MUTATIONS = ("radtan_4_steps", "p1_p2_swapped", "k2_k3_swapped", "t8_is_t4_t2", "newton_468", "no_clamp", "R_transposed",
             "E_with_Rt", "pixel_unit_cam0_only", "no_float_rounding")

# conditioning rule of the GPU tests: a point is ill conditioned when pi/2 - theta < 1e-6, or the Newton denominator is
# below 1e-3, or radtan's 1 + (k2 r2 + k1) r2 is below 1e-3
COND_THETA, COND_DENOM = LD("1e-6"), LD("1e-3")


def _ld(a):
    return np.asarray(a, dtype=LD)


def _pts(pts):
    """Float32 points widened exactly (long-double input is taken as it is: only stereo_guess hands that in)."""
    p = np.asarray(pts)
    if p.dtype != LD:
        p = np.ascontiguousarray(p, dtype=np.float32)
    p = p.reshape(-1, 2)
    return p[:, 0].astype(LD), p[:, 1].astype(LD)


def kb_poly(k, theta, mutate=None):
    """(theta_d, d theta_d / d theta) of the Kannala-Brandt polynomial."""
    t2 = theta * theta
    t4 = t2 * t2
    t6 = t4 * t2
    t8 = t4 * t2 if mutate == "t8_is_t4_t2" else t6 * t2
    a, b, c = (4, 6, 8) if mutate == "newton_468" else (5, 7, 9)
    val = theta * (1 + k[0] * t2 + k[1] * t4 + k[2] * t6 + k[3] * t8)
    der = 1 + 3 * k[0] * t2 + a * k[1] * t4 + b * k[2] * t6 + c * k[3] * t8
    return val, der


def undistort(K, D, model, pts, R=None, mutate=None, info=None):
    """Float32 pixels -> normalised (rotated) coordinates, long double, unrounded, (n, 2).

    info: a dict that receives, per point, what the point went through (reference quantities only):
      equidistant: theta_d, theta, floor, clamp, steps (Newton steps taken, 0 at the floor), exhausted (the tenth step did
      not meet the stop rule), denom (smallest |Newton denominator|), tan_inverted (theta > pi/4);
      radtan: denom (smallest 1 + (k2 r2 + k1) r2 over the five steps);
      both: well (the conditioning rule above)."""
    fx, fy, cx, cy = (LD(v) for v in K)
    k = [LD(v) for v in D]
    u, v = _pts(pts)
    x, y = (u - cx) / fx, (v - cy) / fy
    n = len(x)
    rec = {}
    if model == EQUIDISTANT:
        if mutate == "k2_k3_swapped":
            k[2], k[3] = k[3], k[2]
        r = np.sqrt(x * x + y * y)
        clamp = r > HALF_PI_CLAMP
        theta_d = r if mutate == "no_clamp" else np.where(clamp, HALF_PI_CLAMP, r)
        floor = ~(theta_d > FLOOR)
        theta = theta_d.copy()
        active = ~floor
        steps = np.zeros(n, np.int64)
        denom = np.full(n, LD(1))
        for _ in range(10):
            if not active.any():
                break
            val, der = kb_poly(k, theta, mutate)
            fix = (val - theta_d) / der
            theta = np.where(active, theta - fix, theta)
            denom = np.where(active, np.minimum(denom, np.abs(der)), denom)
            steps += active
            active = active & ~(np.abs(fix) < NEWTON_STOP)
        with np.errstate(divide="ignore", invalid="ignore"):
            scale = np.where(floor, LD(0), np.tan(theta) / np.where(floor, LD(1), theta_d))
        x, y = x * scale, y * scale
        rec = dict(theta_d=theta_d, theta=theta, floor=floor, clamp=clamp, steps=steps, exhausted=active, denom=denom,
                   tan_inverted=~floor & (theta > HALF_PI / 2),
                   well=floor | ((HALF_PI - theta >= COND_THETA) & (denom >= COND_DENOM)))
    else:
        k1, k2, p1, p2 = k
        if mutate == "p1_p2_swapped":
            p1, p2 = p2, p1
        x0, y0 = x, y
        denom = np.full(n, LD(1))
        for _ in range(4 if mutate == "radtan_4_steps" else 5):
            r2 = x * x + y * y
            den = 1 + (k2 * r2 + k1) * r2
            dx = 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
            dy = p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
            x, y = (x0 - dx) / den, (y0 - dy) / den
            denom = np.minimum(denom, den)
        rec = dict(denom=denom, well=denom >= COND_DENOM)
    if R is not None:
        R = _ld(R).reshape(3, 3)
        if mutate == "R_transposed":
            R = R.T
        X = R[0, 0] * x + R[0, 1] * y + R[0, 2]
        Y = R[1, 0] * x + R[1, 1] * y + R[1, 2]
        W = R[2, 0] * x + R[2, 1] * y + R[2, 2]
        x, y = X / W, Y / W
    if info is not None:
        info.update(rec)
    return np.stack([x, y], 1)


def atan_interval(r):
    """(inverted, interval 0..4) of the argument reduction atan(x) = atan(c) + atan((x - c) / (1 + x c)), x > 1 taken as
    pi/2 - atan(1 / x), c the nearest of 0, 1/4, 1/2, 3/4, 1."""
    r = _ld(r)
    inv = r > 1
    with np.errstate(divide="ignore"):
        a = np.where(inv, 1 / np.where(inv, r, LD(1)), r)
    return inv, sum((a > LD(b)).astype(np.int64) for b in ATAN_BOUNDS)


def distort(K, D, model, xy, mutate=None, info=None):
    """Float32 normalised coordinates (the ray (x, y, 1)) -> pixels, long double, unrounded, (n, 2)."""
    fx, fy, cx, cy = (LD(v) for v in K)
    k = [LD(v) for v in D]
    x, y = _pts(xy)
    if model == EQUIDISTANT:
        if mutate == "k2_k3_swapped":
            k[2], k[3] = k[3], k[2]
        r = np.sqrt(x * x + y * y)
        theta = np.arctan(r)
        theta_d, _ = kb_poly(k, theta, mutate)
        big = r > FLOOR
        scale = np.where(big, theta_d / np.where(big, r, LD(1)), LD(1))
        xd, yd = x * scale, y * scale
        if info is not None:
            inv, iv = atan_interval(r)
            info.update(r=r, atan_inverted=inv, atan_interval=iv, floor=~big)
    else:
        k1, k2, p1, p2 = k
        if mutate == "p1_p2_swapped":
            p1, p2 = p2, p1
        r2 = x * x + y * y
        cd = 1 + k1 * r2 + k2 * r2 * r2
        xd = x * cd + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
        yd = y * cd + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
    return np.stack([xd * fx + cx, yd * fy + cy], 1)


def skew(t):
    x, y, z = t
    return np.array([[0, -z, y], [z, 0, -x], [-y, x, 0]], dtype=LD)


def extrinsics(calib, stereo_threshold=5.0, mutate=None):
    """R_cam0_cam1, t_cam0_cam1, E = [t]x R and epi_thresh = stereo_threshold * 4 / (fx0 + fy0 + fx1 + fy1), from
    T_cam0_imu / T_cam1_cam0 (row-major [R t; 0 1]) by the statements of mskf_stream_create."""
    T0 = _ld(list(calib.T_cam0_imu)).reshape(4, 4)
    T10 = _ld(list(calib.T_cam1_cam0)).reshape(4, 4)
    R_cam0_imu = T0[:3, :3].T
    t_cam0_imu = -(R_cam0_imu @ T0[:3, 3])
    T1 = T10 @ T0                                        # T_cam1_imu as the 4 x 4 product
    R_cam1_imu = T1[:3, :3].T
    t_cam1_imu = -(R_cam1_imu @ T1[:3, 3])
    R = R_cam1_imu.T @ R_cam0_imu
    t = R_cam1_imu.T @ (t_cam0_imu - t_cam1_imu)
    E = skew(t) @ (R.T if mutate == "E_with_Rt" else R)
    K0, K1 = [LD(v) for v in calib.cam0_intrinsics], [LD(v) for v in calib.cam1_intrinsics]
    unit = 4 / (K0[0] + K0[1] + K0[0] + K0[1]) if mutate == "pixel_unit_cam0_only" else 4 / (K0[0] + K0[1] + K1[0] + K1[1])
    return dict(R=R, t=t, E=E, epi_thresh=LD(stereo_threshold) * unit)


def cams(calib):
    return ((list(calib.cam0_intrinsics), list(calib.cam0_distortion), int(calib.cam0_model)),
            (list(calib.cam1_intrinsics), list(calib.cam1_distortion), int(calib.cam1_model)))


def stereo_guess(calib, pts, mutate=None, info=None):
    """distort(cam1, float32(undistort(cam0, R_cam0_cam1, pts))): long double pixels in cam1.  info receives `und` (the
    rotated cam0 ray before the rounding), `cam0` (undistort's info) and `cam1` (distort's info)."""
    (K0, D0, m0), (K1, D1, m1) = cams(calib)
    R = extrinsics(calib)["R"]
    i0, i1 = {}, {}
    und = undistort(K0, D0, m0, pts, R=R, mutate=mutate, info=i0)
    mid = und if mutate == "no_float_rounding" else und.astype(np.float32).astype(LD)
    out = distort(K1, D1, m1, mid, mutate=mutate, info=i1)
    if info is not None:
        info.update(und=und, cam0=i0, cam1=i1)
    return out


def epipolar_error(E, und0, und1):
    """|p1^T E p0| / sqrt(l0^2 + l1^2), l = E p0, p = (x, y, 1) of float32 undistorted points, in long double."""
    E = _ld(E).reshape(3, 3)
    x0, y0 = _pts(und0)
    x1, y1 = _pts(und1)
    l0 = E[0, 0] * x0 + E[0, 1] * y0 + E[0, 2]
    l1 = E[1, 0] * x0 + E[1, 1] * y0 + E[1, 2]
    l2 = E[2, 0] * x0 + E[2, 1] * y0 + E[2, 2]
    return np.abs(x1 * l0 + y1 * l1 + l2) / np.sqrt(l0 * l0 + l1 * l1)


def _ordered(f32):
    """float32 -> int64 that orders like the floats (+0 and -0 both 0)."""
    b = np.ascontiguousarray(f32, dtype=np.float32).view(np.int32).astype(np.int64)
    return np.where(b < 0, -(b & 0x7fffffff), b)


def ulps32(got_f32, ref_ld):
    """(distance in float32 ulps between got and the float32 nearest ref, margin): margin = how far ref lies from the
    rounding boundary between that float32 and its neighbour, in ulps (0 = a tie, 0.5 = ref is a float32 itself).  A NaN
    or infinite `got`, or a non-finite ref, counts as a distance of 2^31."""
    got = np.ascontiguousarray(got_f32, dtype=np.float32)
    ref = _ld(ref_ld)
    with np.errstate(over="ignore", invalid="ignore"):
        r32 = ref.astype(np.float32)
    bad = ~np.isfinite(got) | ~np.isfinite(r32)
    dist = np.where(bad, np.int64(1) << 31, np.abs(_ordered(got) - _ordered(r32)))
    with np.errstate(invalid="ignore", over="ignore"):
        off = np.abs(ref - r32.astype(LD))
        toward = np.where(np.abs(ref) >= np.abs(r32.astype(LD)), np.float32(np.inf), np.float32(0)).astype(np.float32)
        nb = np.nextafter(r32, np.copysign(toward, r32))
        ulp = np.abs(nb.astype(LD) - r32.astype(LD))
        margin = np.where(bad | (ulp == 0), LD(0), LD("0.5") - off / np.where(ulp == 0, LD(1), ulp))
    return dist, margin.astype(np.float64)
