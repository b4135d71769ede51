"""Two references for the opt-in camera models (csrc/hip/fe_cam_models.h; DESIGN.md section 3, "Extended camera models").

1. The float64 restatement (`undistort64`, `distort64`, `track_flat64`): the contract operation for operation in numpy float64
   (IEEE + - * / sqrt, one rounding each, like the header under -ffp-contract=off), with det_atan / det_tan restated, the two
   base models included (a mixed stream runs them through the extended kernel).  The header and the device must equal it bit
   for bit.

2. The long-double model (`undistort_ld`, `distort_ld`): written from the models' definitions in np.longdouble with the true
   library tan / atan and the closed forms; radtan8's undistortion is the five published fixed-point steps (the procedure is
   the contract, not the exact inverse).  It extends tests/camera_reference.py, whose base models, rotation and ulp measure it
   uses.  `mutate` switches in one deliberate mistake at a time.

  radtan8  k1 k2 p1 p2 k3 k4 k5 k6.  distort: r2 = x^2 + y^2, radial = (1 + k1 r2 + k2 r2^2 + k3 r2^3) / (1 + k4 r2 + k5 r2^2 +
           k6 r2^3), xd = x radial + 2 p1 x y + p2 (r2 + 2 x^2), yd = y radial + p1 (r2 + 2 y^2) + 2 p2 x y.  undistort: five
           steps (x, y) <- ((x0, y0) - tangential(x, y)) (1 + ((k6 r2 + k5) r2 + k4) r2) / (1 + ((k3 r2 + k2) r2 + k1) r2).
  fov      w.  distort: ru = |(x, y)|, rd = atan(2 ru tan(w / 2)) / w, scale rd / ru (ru < 1e-8: 2 tan(w / 2) / w).  undistort:
           rd = |(xd, yd)|, outside when rd w >= pi/2 (the double), ru = tan(rd w) / (2 tan(w / 2)), scale ru / rd (rd < 1e-8:
           w / (2 tan(w / 2))).
  ds       xi, alpha.  distort: d1 = sqrt(r2 + 1), k = xi d1 + 1, d2 = sqrt(r2 + k^2), den = alpha d2 + (1 - alpha) k, (x, y) /
           den; outside when 1 > -w2 d1 fails (w1 = alpha / (1 - alpha) for alpha <= 0.5 else (1 - alpha) / alpha, w2 = (w1 +
           xi) / sqrt(2 w1 xi + xi^2 + 1)) or den <= 0.  undistort: outside when alpha > 0.5 and r2 > 1 / (2 alpha - 1);
           s = sqrt(max(0, 1 - (2 alpha - 1) r2)), mz = (1 - alpha^2 r2) / (alpha s + 1 - alpha), t = (mz xi + sqrt(mz^2 +
           (1 - xi^2) r2)) / (mz^2 + r2), ray (t mx, t my, t mz - xi); outside when its z <= 0 (or no number); divide by z.
"""
import numpy as np

import camera_reference as R

LD = R.LD
F64 = np.float64
RADTAN, EQUIDISTANT, RADTAN8, FOV, DS = 0, 1, 2, 3, 4
MODEL_NAMES = {RADTAN: "radtan", EQUIDISTANT: "equidistant", RADTAN8: "radtan8", FOV: "fov", DS: "ds"}
FLOOR = 1e-8
HALF_PI = 1.5707963267948966

MUTATIONS = ("k3_k4_swapped", "rational_inverted", "alpha_for_one_minus_alpha", "xi_sign", "no_minus_xi", "w_for_half_w", "p1_p2_swapped")
MUTATION_MODEL = dict(k3_k4_swapped=RADTAN8, rational_inverted=RADTAN8, p1_p2_swapped=RADTAN8, alpha_for_one_minus_alpha=DS,
                      xi_sign=DS, no_minus_xi=DS, w_for_half_w=FOV)

# conditioning rule of the GPU test (long-double quantities): a coordinate is ill conditioned when
#   fov undistort: |pi/2 - rd w| < 1e-6 (tan's pole, and the domain's edge from either side);
#   ds undistort:  |1 - (2 alpha - 1) r2| < 1e-6 (alpha > 0.5), or, inside that edge, the ray's |z| < 1e-3 or |alpha s + 1 - alpha| < 1e-3;
#   ds distort:    |den| < 1e-3, or |1 + w2 d1| < 1e-6;
#   radtan8:       numerator or denominator of the rational factor below 1e-3;
#   through R:     the rotated ray's |W| < 1e-3 (a ray near 90 degrees off cam1's axis).
# The edges are two-sided, so a point that double and long double could classify differently is never judged.
COND_EDGE, COND_DENOM = LD("1e-6"), LD("1e-3")


def coeffs8(model, coeffs):
    k = [float(v) for v in coeffs]
    return k + [0.0] * (8 - len(k))


# ------------------------------------------------------------------------------------------ float64 restatement
def det_atan64(x):
    x = np.asarray(x, F64).copy()
    inv = x > 1.0
    with np.errstate(divide="ignore"):
        x = np.where(inv, 1.0 / np.where(inv, x, 1.0), x)
    c = np.zeros_like(x)
    ac = np.zeros_like(x)
    for lo, cv, acv in ((0.125, 0.25, 0.24497866312686415417), (0.375, 0.5, 0.46364760900080611621),
                        (0.625, 0.75, 0.64350110879328438680), (0.875, 1.0, 0.78539816339744830962)):
        m = x > lo
        c = np.where(m, cv, c)
        ac = np.where(m, acv, ac)
    z = (x - c) / (1.0 + x * c)
    z2 = z * z
    p = np.full_like(x, 1.0 / 21.0)
    for d in (19.0, 17.0, 15.0, 13.0, 11.0, 9.0, 7.0, 5.0, 3.0):
        p = 1.0 / d - z2 * p
    p = 1.0 - z2 * p
    a = ac + z * p
    return np.where(inv, 1.5707963267948966192 - a, a)


def det_tan64(t):
    t = np.asarray(t, F64).copy()
    inv = t > 0.78539816339744830962
    t = np.where(inv, (1.5707963267948966192 - t) + 6.123233995736766e-17, t)
    t2 = t * t
    s = np.full_like(t, 1.0 / 121645100408832000.0)
    for d in (355687428096000.0, 1307674368000.0, 6227020800.0, 39916800.0, 362880.0, 5040.0, 120.0, 6.0):
        s = 1.0 / d - t2 * s
    s = t * (1.0 - t2 * s)
    c = np.full_like(t, 1.0 / 6402373705728000.0)
    for d in (20922789888000.0, 87178291200.0, 479001600.0, 3628800.0, 40320.0, 720.0, 24.0):
        c = 1.0 / d - t2 * c
    c = 0.5 - t2 * c
    c = 1.0 - t2 * c
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(inv, c / s, s / c)


def _model_undistort64(model, k, x, y):
    """Normalised distorted -> normalised undistorted, float64 arrays; returns (x, y, ok)."""
    n = len(x)
    ok = np.ones(n, bool)
    with np.errstate(all="ignore"):
        if model == RADTAN:
            k1, k2, p1, p2 = k[:4]
            x0, y0 = x, y
            for _ in range(5):
                r2 = x * x + y * y
                icdist = 1.0 / (1.0 + (k2 * r2 + k1) * r2)
                dx = 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
                dy = p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
                x, y = (x0 - dx) * icdist, (y0 - dy) * icdist
        elif model == EQUIDISTANT:
            theta_d = np.sqrt(x * x + y * y)
            theta_d = np.where(theta_d > HALF_PI, HALF_PI, theta_d)
            big = theta_d > 1e-8
            theta = theta_d.copy()
            active = big.copy()
            for _ in range(10):
                t2 = theta * theta
                t4 = t2 * t2
                t6 = t4 * t2
                t8 = t6 * t2
                a, b, c, d = k[0] * t2, k[1] * t4, k[2] * t6, k[3] * t8
                fix = (theta * (1 + a + b + c + d) - theta_d) / (1 + 3 * a + 5 * b + 7 * c + 9 * d)
                theta = np.where(active, theta - fix, theta)
                active = active & ~(np.abs(fix) < 1e-8)
            scale = np.where(big, det_tan64(theta) / np.where(big, theta_d, 1.0), 0.0)
            x, y = x * scale, y * scale
        elif model == RADTAN8:
            k1, k2, p1, p2, k3, k4, k5, k6 = k
            x0, y0 = x, y
            for _ in range(5):
                r2 = x * x + y * y
                icdist = (1.0 + ((k6 * r2 + k5) * r2 + k4) * r2) / (1.0 + ((k3 * r2 + k2) * r2 + k1) * r2)
                dx = 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
                dy = p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
                x, y = (x0 - dx) * icdist, (y0 - dy) * icdist
        elif model == FOV:
            w = F64(k[0])
            two_tw = 2.0 * det_tan64(np.array([w * 0.5]))[0]
            rd = np.sqrt(x * x + y * y)
            a = rd * w
            ok = a < HALF_PI
            small = rd < FLOOR
            ru = det_tan64(np.where(ok, a, 0.0)) / two_tw
            scale = np.where(small, w / two_tw, ru / np.where(small, 1.0, rd))
            x, y = x * scale, y * scale
        elif model == DS:
            xi, alpha = F64(k[0]), F64(k[1])
            mx, my = x, y
            r2 = mx * mx + my * my
            b = 2.0 * alpha - 1.0
            if alpha > 0.5:
                ok = ~(r2 > 1.0 / b)
            sa = 1.0 - b * r2
            sa = np.where(sa < 0.0, 0.0, sa)
            s = np.sqrt(sa)
            mz = (1.0 - alpha * alpha * r2) / (alpha * s + 1.0 - alpha)
            mz2 = mz * mz
            t = (mz * xi + np.sqrt(mz2 + (1.0 - xi * xi) * r2)) / (mz2 + r2)
            rz = t * mz - xi
            ok = ok & (rz > 0.0)
            x, y = t * mx / rz, t * my / rz
        else:
            raise ValueError(model)
    return x, y, ok


def undistort64(K, model, coeffs, px, Rm=None):
    """float32 pixels -> (float32 normalised coordinates (n, 2), in-domain flags): undistort_pt / fcm_undistort_px.  Outside the
    domain the coordinates are 0."""
    fx, fy, cx, cy = (F64(v) for v in K)
    k = [F64(v) for v in coeffs8(model, coeffs)]
    p = np.ascontiguousarray(px, np.float32).reshape(-1, 2)
    x = (p[:, 0].astype(F64) - cx) / fx
    y = (p[:, 1].astype(F64) - cy) / fy
    x, y, ok = _model_undistort64(model, k, x, y)
    with np.errstate(all="ignore"):
        if Rm is not None:
            r = np.asarray(Rm, F64).reshape(9)
            X = r[0] * x + r[1] * y + r[2]
            Y = r[3] * x + r[4] * y + r[5]
            W = r[6] * x + r[7] * y + r[8]
            x, y = X / W, Y / W
        else:
            x, y = x / 1.0, y / 1.0
        out = np.stack([x * 1.0 + 0.0, y * 1.0 + 0.0], 1).astype(np.float32)          # (P = {1, 1, 0, 0}: the + 0.0 turns a -0 into +0)
    out[~ok] = 0
    return out, ok


def distort64(K, model, coeffs, xy):
    """float32 rays (x, y, 1) -> (float32 pixels, in-domain flags): distort_pt / fcm_distort_px."""
    fx, fy, cx, cy = (F64(v) for v in K)
    k = [F64(v) for v in coeffs8(model, coeffs)]
    p = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
    x, y = p[:, 0].astype(F64), p[:, 1].astype(F64)
    ok = np.ones(len(x), bool)
    with np.errstate(all="ignore"):
        if model == RADTAN:
            k1, k2, p1, p2 = k[:4]
            r2 = x * x + y * y
            r4 = r2 * r2
            a1, a2, a3 = 2.0 * x * y, r2 + 2.0 * x * x, r2 + 2.0 * y * y
            cdist = 1.0 + k1 * r2 + k2 * r4
            xd, yd = x * cdist + p1 * a1 + p2 * a2, y * cdist + p1 * a3 + p2 * a1
        elif model == EQUIDISTANT:
            r = np.sqrt(x * x + y * y)
            theta = det_atan64(r)
            t2 = theta * theta
            t4 = t2 * t2
            t6 = t4 * t2
            t8 = t4 * t4
            theta_d = theta * (1 + k[0] * t2 + k[1] * t4 + k[2] * t6 + k[3] * t8)
            big = r > 1e-8
            scale = np.where(big, theta_d / np.where(big, r, 1.0), 1.0)
            xd, yd = x * scale, y * scale
        elif model == RADTAN8:
            k1, k2, p1, p2, k3, k4, k5, k6 = k
            r2 = x * x + y * y
            r4 = r2 * r2
            r6 = r4 * r2
            a1, a2, a3 = 2.0 * x * y, r2 + 2.0 * x * x, r2 + 2.0 * y * y
            cdist = 1.0 + k1 * r2 + k2 * r4 + k3 * r6
            icdist2 = 1.0 / (1.0 + k4 * r2 + k5 * r4 + k6 * r6)
            xd, yd = x * cdist * icdist2 + p1 * a1 + p2 * a2, y * cdist * icdist2 + p1 * a3 + p2 * a1
        elif model == FOV:
            w = F64(k[0])
            two_tw = 2.0 * det_tan64(np.array([w * 0.5]))[0]
            ru = np.sqrt(x * x + y * y)
            small = ru < FLOOR
            rd = det_atan64(two_tw * ru) / w
            scale = np.where(small, two_tw / w, rd / np.where(small, 1.0, ru))
            xd, yd = x * scale, y * scale
        elif model == DS:
            xi, alpha = F64(k[0]), F64(k[1])
            r2 = x * x + y * y
            d1 = np.sqrt(r2 + 1.0)
            kk = xi * d1 + 1.0
            d2 = np.sqrt(r2 + kk * kk)
            den = alpha * d2 + (1.0 - alpha) * kk
            w1 = (1.0 - alpha) / alpha if alpha > 0.5 else alpha / (1.0 - alpha)
            w2 = (w1 + xi) / np.sqrt(2.0 * w1 * xi + xi * xi + 1.0)
            ok = (1.0 > -w2 * d1) & (den > 0.0)
            xd, yd = x / den, y / den
        else:
            raise ValueError(model)
        out = np.stack([xd * fx + cx, yd * fy + cy], 1).astype(np.float32)
    out[~ok] = 0
    return out, ok


def track_flat64(cam0, cam1, R01, pts):
    """What a stereo-only track call returns on a flat pair (no pyramid level can be solved, so out1 is the stereo guess): dict of
    out0, out1, und0, und1, status.  cam = (K, model, coeffs).  The domain rule: no guess -> no stereo trip, out1 = 0; und0 or und1
    outside -> status bit 1 clear (on a flat pair it is clear anyway) and the coordinates 0."""
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 2)
    ray, ok0 = undistort64(cam0[0], cam0[1], cam0[2], pts, Rm=R01)
    guess, ok1 = distort64(cam1[0], cam1[1], cam1[2], ray)
    guessed = ok0 & ok1
    out1 = np.where(guessed[:, None], guess, np.float32(0)).astype(np.float32)
    und0, _ = undistort64(cam0[0], cam0[1], cam0[2], pts)
    und1, _ = undistort64(cam1[0], cam1[1], cam1[2], out1)
    return dict(out0=pts, out1=out1, und0=und0, und1=und1, status=np.ones(len(pts), np.uint8), guessed=guessed)


# ------------------------------------------------------------------------------------------ long-double model
def _pi_half():
    return LD(2) * np.arctan(LD(1))


def undistort_ld(K, model, coeffs, px, Rm=None, mutate=None, info=None):
    """float32 pixels -> (long-double normalised coordinates (n, 2), unrounded; in-domain flags).  info receives `well`."""
    if model in (RADTAN, EQUIDISTANT):
        i = {}
        out = R.undistort(K, list(coeffs)[:4], model, px, R=Rm, info=i)
        if info is not None:
            info.update(well=np.asarray(i["well"]))
        return out, np.ones(len(out), bool)
    fx, fy, cx, cy = (LD(v) for v in K)
    k = [LD(v) for v in coeffs8(model, coeffs)]
    u, v = R._pts(px)
    x, y = (u - cx) / fx, (v - cy) / fy
    n = len(x)
    ok = np.ones(n, bool)
    well = np.ones(n, bool)
    with np.errstate(all="ignore"):
        if model == RADTAN8:
            k1, k2, p1, p2, k3, k4, k5, k6 = k
            if mutate == "k3_k4_swapped":
                k3, k4 = k4, k3
            if mutate == "p1_p2_swapped":
                p1, p2 = p2, p1
            x0, y0 = x, y
            for _ in range(5):
                r2 = x * x + y * y
                num = 1 + ((k6 * r2 + k5) * r2 + k4) * r2
                den = 1 + ((k3 * r2 + k2) * r2 + k1) * r2
                if mutate == "rational_inverted":
                    num, den = den, num
                dx = 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
                dy = p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
                x, y = (x0 - dx) * num / den, (y0 - dy) * num / den
                well &= (np.abs(den) >= COND_DENOM) & (np.abs(num) >= COND_DENOM)
        elif model == FOV:
            w = k[0]
            half = w if mutate == "w_for_half_w" else w / 2
            rd = np.sqrt(x * x + y * y)
            a = rd * w
            ok = a < LD(HALF_PI)
            small = rd < LD(FLOOR)
            ru = np.tan(np.where(ok, a, LD(0))) / (2 * np.tan(half))
            scale = np.where(small, w / (2 * np.tan(half)), ru / np.where(small, LD(1), rd))
            x, y = x * scale, y * scale
            well &= np.abs(_pi_half() - a) >= COND_EDGE
        elif model == DS:
            xi, alpha = k[0], k[1]
            if mutate == "xi_sign":
                xi = -xi
            r2 = x * x + y * y
            b = 2 * alpha - 1
            out1 = np.zeros(n, bool)
            if alpha > LD("0.5"):
                out1 = r2 > 1 / b
                ok = ~out1
                well &= np.abs(1 - b * r2) >= COND_EDGE
            sa = np.maximum(1 - b * r2, LD(0))
            s = np.sqrt(sa)
            one_minus = alpha if mutate == "alpha_for_one_minus_alpha" else 1 - alpha
            dz = alpha * s + one_minus
            mz = (1 - alpha * alpha * r2) / dz
            t = (mz * xi + np.sqrt(mz * mz + (1 - xi * xi) * r2)) / (mz * mz + r2)
            rz = t * mz if mutate == "no_minus_xi" else t * mz - xi
            ok = ok & (rz > 0)
            x, y = t * x / rz, t * y / rz
            well &= out1 | ((np.abs(rz) >= COND_DENOM) & (np.abs(dz) >= COND_DENOM))
        else:
            raise ValueError(model)
        if Rm is not None:
            r = R._ld(Rm).reshape(9)
            X = r[0] * x + r[1] * y + r[2]
            Y = r[3] * x + r[4] * y + r[5]
            W = r[6] * x + r[7] * y + r[8]
            x, y = X / W, Y / W
            well &= ~ok | (np.abs(W) >= COND_DENOM)
    if info is not None:
        info.update(well=well)
    return np.stack([x, y], 1), ok


def distort_ld(K, model, coeffs, xy, mutate=None, info=None):
    """float32 (or long-double) rays -> (long-double pixels (n, 2), unrounded; in-domain flags).  info receives `well`."""
    if model in (RADTAN, EQUIDISTANT):
        out = R.distort(K, list(coeffs)[:4], model, xy)
        if info is not None:
            info.update(well=np.ones(len(out), bool))
        return out, np.ones(len(out), bool)
    fx, fy, cx, cy = (LD(v) for v in K)
    k = [LD(v) for v in coeffs8(model, coeffs)]
    x, y = R._pts(xy)
    n = len(x)
    ok = np.ones(n, bool)
    well = np.ones(n, bool)
    with np.errstate(all="ignore"):
        if model == RADTAN8:
            k1, k2, p1, p2, k3, k4, k5, k6 = k
            if mutate == "k3_k4_swapped":
                k3, k4 = k4, k3
            if mutate == "p1_p2_swapped":
                p1, p2 = p2, p1
            r2 = x * x + y * y
            num = 1 + k1 * r2 + k2 * r2 * r2 + k3 * r2 * r2 * r2
            den = 1 + k4 * r2 + k5 * r2 * r2 + k6 * r2 * r2 * r2
            if mutate == "rational_inverted":
                num, den = den, num
            rad = num / den
            xd = x * rad + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
            yd = y * rad + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
            well &= np.abs(den) >= COND_DENOM
        elif model == FOV:
            w = k[0]
            half = w if mutate == "w_for_half_w" else w / 2
            ru = np.sqrt(x * x + y * y)
            small = ru < LD(FLOOR)
            rd = np.arctan(2 * ru * np.tan(half)) / w
            scale = np.where(small, 2 * np.tan(half) / w, rd / np.where(small, LD(1), ru))
            xd, yd = x * scale, y * scale
        elif model == DS:
            xi, alpha = k[0], k[1]
            if mutate == "xi_sign":
                xi = -xi
            r2 = x * x + y * y
            d1 = np.sqrt(r2 + 1)
            kk = xi * d1 + 1
            d2 = np.sqrt(r2 + kk * kk)
            one_minus = alpha if mutate == "alpha_for_one_minus_alpha" else 1 - alpha
            den = alpha * d2 + one_minus * kk
            w1 = (1 - alpha) / alpha if alpha > LD("0.5") else alpha / (1 - alpha)
            w2 = (w1 + xi) / np.sqrt(2 * w1 * xi + xi * xi + 1)
            ok = (1 > -w2 * d1) & (den > 0)
            xd, yd = x / den, y / den
            well &= (np.abs(den) >= COND_DENOM) & (np.abs(1 + w2 * d1) >= COND_EDGE)
        else:
            raise ValueError(model)
    if info is not None:
        info.update(well=well)
    return np.stack([xd * fx + cx, yd * fy + cy], 1), ok


def exact_undistort_ld(K, model, coeffs, px, steps=60):
    """radtan8's exact inverse, by the fixed-point iteration run until it no longer moves (for the report of what five steps leave)."""
    fx, fy, cx, cy = (LD(v) for v in K)
    k1, k2, p1, p2, k3, k4, k5, k6 = (LD(v) for v in coeffs8(model, coeffs))
    u, v = R._pts(px)
    x0, y0 = (u - cx) / fx, (v - cy) / fy
    x, y = x0, y0
    for _ in range(steps):
        r2 = x * x + y * y
        ic = (1 + ((k6 * r2 + k5) * r2 + k4) * r2) / (1 + ((k3 * r2 + k2) * r2 + k1) * r2)
        dx = 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
        dy = p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
        x, y = (x0 - dx) * ic, (y0 - dy) * ic
    return np.stack([x, y], 1)
