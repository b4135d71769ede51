"""Seeded calibrations and point sets that drive the per-point camera geometry of k_track4 (undistort_pt, distort_pt, the
stereo guess through R_cam0_cam1, the epipolar gate) at the edges of the two camera models, and helpers that say, from the
long-double reference alone (tests/camera_reference.py), which branch every point takes and whether it is well conditioned.

A case is (pair name, extrinsics name): calib(pair, ext) is the mskf_calib, point_set(pair, ext) its cam0 pixels (float32,
at most MAX_POINTS: one track call of a default stream) with a label per point naming the subset it belongs to.  The cam1
side is reached through the stereo guess: the cam0 pixel of a wanted cam1 ray comes from the long-double forward model.

tests/test_camera_reference.py holds the conditions that keep these sets from degenerating (no GPU);
tests/test_gpu_camera_geometry.py runs them on the device.
"""
import math

import numpy as np

import camera_reference as R
from camera_reference import EQUIDISTANT, LD, RADTAN

MAX_POINTS = 1500
ULP_CAP_SHARE = 1e-3        # at most 0.1 % of a set's well-conditioned coordinates may differ from the rounded reference, by 1 ulp
ILL_CAP_SHARE = 0.02        # at most 2 % of a set's points may be ill conditioned


def _cam(K, D, model, size, margin=False):
    return dict(K=tuple(float(v) for v in K), D=tuple(float(v) for v in D), model=model, size=size, margin=margin)


EUROC0_K, EUROC1_K = (458.654, 457.296, 367.215, 248.375), (457.587, 456.134, 379.999, 255.238)
MILD = (-0.013, 0.021, -0.008, 0.0015)
CAMERAS = dict(
    # EuRoC MAV dataset, radtan (published calibration)
    euroc0=_cam(EUROC0_K, (-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05), RADTAN, (752, 480), True),
    euroc1=_cam(EUROC1_K, (-0.28368365, 0.07451284, -0.00010473, -3.55590700e-05), RADTAN, (752, 480), True),
    # the mild Kannala-Brandt set of the LK tests, on the EuRoC intrinsics
    mild0=_cam(EUROC0_K, MILD, EQUIDISTANT, (752, 480), True),
    mild1=_cam(EUROC1_K, tuple(0.9 * v for v in MILD), EQUIDISTANT, (752, 480), True),
    # TUM-VI-like 512 x 512 fisheye (195 degrees: the corners lie outside the image circle)
    tumvi0=_cam((190.98, 190.97, 254.93, 256.90), (0.003482, 0.000715, -0.002053, 0.000203), EQUIDISTANT, (512, 512)),
    tumvi1=_cam((190.44, 190.43, 252.59, 254.91), (0.003400, 0.001766, -0.002663, 0.000330), EQUIDISTANT, (512, 512)),
    # Kalibr-like strong set: the polynomial turns over inside the sensor, Newton runs out of its ten steps there
    kalibr0=_cam((380.8, 380.7, 365.8, 254.3), (0.0102, -0.0088, 0.0182, -0.0107), EQUIDISTANT, (752, 480)),
    kalibr1=_cam((379.9, 380.2, 370.1, 250.6), (0.0098, -0.0081, 0.0171, -0.0101), EQUIDISTANT, (752, 480)),
    # the ideal equidistant lens of a simulator, float-representable intrinsics
    ideal0=_cam((140.0, 140.0, 320.0, 240.0), (0, 0, 0, 0), EQUIDISTANT, (640, 480)),
    ideal1=_cam((142.0, 141.0, 318.0, 242.0), (0, 0, 0, 0), EQUIDISTANT, (640, 480)),
    # positive coefficients: at the clamp theta_d = pi/2 the ray angle is 1.3 rad, a well-conditioned clamped point
    kbpos0=_cam((140.0, 140.0, 320.0, 240.0), (0.08, 0.01, 0.002, 0.0005), EQUIDISTANT, (640, 480)),
    kbpos1=_cam((141.0, 139.5, 321.5, 238.5), (0.07, 0.012, 0.0015, 0.0006), EQUIDISTANT, (640, 480)),
    # ideal lenses whose principal point lies 1.2e-6 / 1.6e-6 px beside the pixel (320, 240): theta_d of that pixel is
    # 0.86e-8 (under the 1e-8 floor) / 1.14e-8 (over it)
    under=_cam((140.0, 140.0, 320.0 + 1.2e-6, 240.0), (0, 0, 0, 0), EQUIDISTANT, (640, 480)),
    over=_cam((140.0, 140.0, 320.0 + 1.6e-6, 240.0), (0, 0, 0, 0), EQUIDISTANT, (640, 480)),
    # radtan with all coefficients zero (undistort is the identity map) and with dominant tangential terms
    zero0=_cam((460.0, 455.0, 376.0, 240.0), (0, 0, 0, 0), RADTAN, (752, 480), True),
    zero1=_cam((458.0, 457.0, 380.0, 244.0), (0, 0, 0, 0), RADTAN, (752, 480), True),
    tang0=_cam((420.0, 425.0, 370.5, 245.25), (-0.05, 0.01, 0.012, -0.009), RADTAN, (752, 480), True),
    tang1=_cam((422.0, 424.0, 372.25, 243.5), (-0.045, 0.008, -0.011, 0.010), RADTAN, (752, 480), True),
)
PAIRS = dict(euroc=("euroc0", "euroc1"), mild=("mild0", "mild1"), tumvi=("tumvi0", "tumvi1"), kalibr=("kalibr0", "kalibr1"),
             ideal=("ideal0", "ideal1"), kbpos=("kbpos0", "kbpos1"), floor_under=("under", "over"), floor_over=("over", "under"),
             zero=("zero0", "zero1"), tang=("tang0", "tang1"), radtan_equi=("euroc0", "mild1"), equi_radtan=("mild0", "euroc1"))


def _rot(axis, deg):
    a = math.radians(deg)
    c, s = math.cos(a), math.sin(a)
    return {"x": np.array([[1.0, 0, 0], [0, c, -s], [0, s, c]]), "y": np.array([[c, 0, s], [0, 1.0, 0], [-s, 0, c]]),
            "z": np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]])}[axis]


def _T(Rm, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = Rm, t
    return T


EUROC_T_CAM0_IMU = np.array([0.014865542981794, 0.999557249008346, -0.025774436697440, 0.065222909535531,
                             -0.999880929698575, 0.014967213324719, 0.003756188357967, -0.020706385492719,
                             0.004140296794224, 0.025715529947966, 0.999660727177902, -0.008054602460030,
                             0, 0, 0, 1.0]).reshape(4, 4)
EUROC_T_CAM1_CAM0 = np.array([0.999997256477881, 0.002312067192424, 0.000376008102415, -0.110073808127187,
                              -0.002317135723281, 0.999898048506644, 0.014089835846648, 0.000399121547014,
                              -0.000343393120525, -0.014090668452714, 0.999900662637729, -0.000853702503357,
                              0, 0, 0, 1.0]).reshape(4, 4)
GENERAL_T_CAM0_IMU = _T(_rot("z", 31.0) @ _rot("x", 19.0) @ _rot("y", -11.0), [0.05, -0.02, 0.01])
# name -> (T_cam0_imu, T_cam1_cam0); T_cam0_imu is a general rotation everywhere, so R_cam1_imu^T R_cam0_imu is a real product
EXTRINSICS = dict(
    identity=(GENERAL_T_CAM0_IMU, _T(np.eye(3), [-0.11, 0.0, 0.0])),
    euroc=(EUROC_T_CAM0_IMU, EUROC_T_CAM1_CAM0),
    verged=(GENERAL_T_CAM0_IMU, _T(_rot("y", 7.0) @ _rot("x", -4.0), [-0.10, 0.002, 0.01])),
    roll90=(GENERAL_T_CAM0_IMU, _T(_rot("z", 90.0), [-0.10, 0.0, 0.0])),
    vertical=(GENERAL_T_CAM0_IMU, _T(_rot("x", 0.5), [0.001, -0.12, 0.002])),
    verged05=(GENERAL_T_CAM0_IMU, _T(_rot("y", 0.5), [-0.11, 0.001, 0.0])),
)
# the cases of the flat-image probe: every pair once, and the two real-lens families under every kind of extrinsics
FLAT_CASES = [("euroc", "euroc"), ("mild", "verged"), ("tumvi", "roll90"), ("kalibr", "vertical"), ("ideal", "identity"),
              ("kbpos", "verged"), ("floor_under", "identity"), ("floor_over", "identity"), ("zero", "roll90"),
              ("tang", "vertical"), ("radtan_equi", "verged"), ("equi_radtan", "euroc"),
              ("euroc", "identity"), ("euroc", "verged"), ("euroc", "roll90"), ("euroc", "vertical"),
              ("tumvi", "identity"), ("tumvi", "euroc"), ("tumvi", "verged"), ("tumvi", "vertical"), ("ideal", "verged")]


def calib(pair, ext, width=None, height=None):
    """The mskf_calib of a case; width / height default to the sensor of cam0 (the intrinsics do not depend on them)."""
    from msckf_stereo_c_amd.ctypes_types import Calib
    c0, c1 = (CAMERAS[n] for n in PAIRS[pair])
    c = Calib()
    c.width, c.height = (width or c0["size"][0]), (height or c0["size"][1])
    for i in range(4):
        c.cam0_intrinsics[i], c.cam0_distortion[i] = c0["K"][i], c0["D"][i]
        c.cam1_intrinsics[i], c.cam1_distortion[i] = c1["K"][i], c1["D"][i]
    c.cam0_model, c.cam1_model = c0["model"], c1["model"]
    T0, T10 = EXTRINSICS[ext]
    for i in range(16):
        c.T_cam0_imu[i], c.T_cam1_cam0[i] = T0.flat[i], T10.flat[i]
        c.T_imu_body[i] = np.eye(4).flat[i]
    return c


# ---------------------------------------------------------------------------------------------- points
def _f32_ulp_steps(v, steps):
    """The float32 values `steps` ulps away from float32(v) (negative: towards zero for positive v)."""
    out = []
    for s in steps:
        x = np.float32(v)
        for _ in range(abs(s)):
            x = np.nextafter(x, np.float32(np.inf if s > 0 else -np.inf))
        out.append(float(x))
    return out


DIRS = [(0.0, 1.0), (1.0, 0.0), (-0.6, 0.8), (0.28, -0.96)]         # exact unit vectors


FIELD_POINTS = 1150


def _field(cam, rng):
    """A grid and a seeded cloud, FIELD_POINTS together, over the sensor (with a 10 % margin where the camera says so).
    Of a fisheye only the part inside the image circle (ray angle under 1.5 rad): the rest of such a sensor sees nothing,
    and the rim has sets of its own."""
    w, h = cam["size"]
    m = 0.1 if cam["margin"] else 0.0
    x0, x1, y0, y1 = -m * w, (w - 1) + m * w, -m * h, (h - 1) + m * h
    gx, gy = np.meshgrid(np.linspace(x0, x1, 26), np.linspace(y0, y1, 20))
    grid = np.stack([gx.ravel(), gy.ravel()], 1).astype(np.float32)
    cloud = np.stack([rng.uniform(x0, x1, 8000), rng.uniform(y0, y1, 8000)], 1).astype(np.float32)
    if cam["model"] == EQUIDISTANT:
        def inside(p):
            info = {}
            R.undistort(cam["K"], cam["D"], cam["model"], p, info=info)
            return p[np.asarray(~info["clamp"] & (info["theta"] < 1.5))]
        grid, cloud = inside(grid), inside(cloud)
    return [("grid", grid), ("cloud", cloud[:FIELD_POINTS - len(grid)])]


def _principal(cam):
    """The principal point, its row and column (where float32 holds cx / cy exactly), and the image corners."""
    fx, fy, cx, cy = cam["K"]
    w, h = cam["size"]
    pts = [(cx, cy)]
    if float(np.float32(cx)) == cx:
        pts += [(cx, v) for v in (0.0, 0.25 * h, 0.5 * h + 3.5, h - 1.0)]
    if float(np.float32(cy)) == cy:
        pts += [(u, cy) for u in (0.0, 0.25 * w, 0.5 * w + 7.25, w - 1.0)]
    corners = [(0.0, 0.0), (w - 1.0, 0.0), (0.0, h - 1.0), (w - 1.0, h - 1.0)]
    return [("principal", np.array(pts, np.float32)), ("corners", np.array(corners, np.float32))]


def _theta_pixels(cam, thetas, dirs=DIRS):
    """Pixels of the rays at the given angles from the axis (long-double forward model), along each direction."""
    fx, fy, cx, cy = (LD(v) for v in cam["K"])
    td, _ = R.kb_poly([LD(v) for v in cam["D"]], np.asarray(thetas, dtype=LD))
    return np.array([(float(cx + fx * t * LD(dx)), float(cy + fy * t * LD(dy))) for (dx, dy) in dirs for t in td], np.float32)


def _undistort_rings(cam):
    """Equidistant, undistort side: theta on each side of pi/4 (tan direct / inverted), theta approaching pi/2 from below,
    theta_d approaching its clamp pi/2 from below down to the last float32 pixel, and at or over the clamp."""
    fx, fy, cx, cy = cam["K"]
    q, hp = math.pi / 4, math.pi / 2
    out = [("tan_quarter", _theta_pixels(cam, [q * (1 - 1e-2), q * (1 - 1e-5), q * (1 + 1e-5), q * (1 + 1e-2)]))]
    near = [t for t in (hp - 1e-2, hp - 1e-4, hp - 2e-6, hp - 5e-7)
            if float(R.kb_poly([LD(v) for v in cam["D"]], LD(t))[0]) < hp]
    if near:
        out.append(("theta_rim", _theta_pixels(cam, near, DIRS[:2])))
    # theta_d = pi/2 along +v and +u: the pixel coordinate at which the clamp sets in, and float32 steps around it
    rim = []
    for (f, c, axis, steps) in ((fy, cy, 1, [-512, -8, -1, 0, 1]), (fx, cx, 0, [-1, 0, 1])):
        edge = c + f * hp
        for val in _f32_ulp_steps(edge, steps) + [edge + 5.0]:
            rim.append((val, cy) if axis == 0 else (cx, val))
    d = 1.5 / math.sqrt(2.0)                                   # diagonals: a shade inside, well outside
    rim += [(cx + fx * d, cy + fy * d), (cx - fx * 1.2, cy + fy * 1.2)]
    out.append(("clamp_rim", np.array(rim, np.float32)))
    return out


def _cam1_ray_pixels(pair, ext, radii, dirs=DIRS):
    """cam0 pixels whose ray, turned into cam1 by R_cam0_cam1, has the given |(x, y)| there (the argument of atan in
    distort_pt): the long-double inverse of the stereo guess' first half."""
    c0 = CAMERAS[PAIRS[pair][0]]
    Rm = R.extrinsics(calib(pair, ext))["R"]
    rays1 = np.array([[LD(r) * LD(dx), LD(r) * LD(dy), LD(1)] for (dx, dy) in dirs for r in radii], dtype=LD)
    rays0 = rays1 @ Rm                                          # R^T applied to each ray
    ok = rays0[:, 2] > LD("0.05")
    xy0 = rays0[ok, :2] / rays0[ok, 2:3]
    return R.distort(c0["K"], c0["D"], c0["model"], xy0).astype(np.float64).astype(np.float32)


ATAN_RING_RADII = [b * s for b in (0.125, 0.375, 0.625, 0.875, 1.0) for s in (1 - 1e-3, 1 - 2e-6, 1 + 2e-6, 1 + 1e-3)]
ATAN_RING_RADII += [s / b for b in (0.125, 0.375, 0.625, 0.875) for s in (1 - 1e-3, 1 - 2e-6, 1 + 2e-6, 1 + 1e-3)]


_SETS = {}


def point_set(pair, ext):
    """(pts float32 n x 2, labels: n subset names) of a case."""
    key = (pair, ext)
    if key not in _SETS:
        c0, c1 = (CAMERAS[n] for n in PAIRS[pair])
        rng = np.random.default_rng(sum(map(ord, pair + ext)))
        parts = _field(c0, rng) + _principal(c0)
        if c0["model"] == EQUIDISTANT:
            parts += _undistort_rings(c0)
            # pixels that the ideal lens clamps to theta_d = the double pi/2 exactly, where tan's reduced argument is smallest
            parts.append(("ideal_rim_clamped", np.array([(320.0, 465.0), (321.0, 465.0), (550.0, 240.0)], np.float32)))
        if c1["model"] == EQUIDISTANT:
            radii = ATAN_RING_RADII if c0["model"] == EQUIDISTANT else [r for r in ATAN_RING_RADII if r < 0.9]
            parts.append(("atan_rings", _cam1_ray_pixels(pair, ext, radii)))
        pts = np.concatenate([p for _, p in parts]).astype(np.float32)
        labels = np.concatenate([[n] * len(p) for n, p in parts])
        assert len(pts) <= MAX_POINTS and np.isfinite(pts).all()
        pts.setflags(write=False)
        _SETS[key] = (pts, labels)
    return _SETS[key]


# ---------------------------------------------------------------------------------------------- what the reference says
def branches(pair, ext, pts=None, guess=None):
    """Per point, from the reference alone: the three stages' branch records.
      und0:  undistort(cam0, p)                       (info of camera_reference.undistort)
      guess: undistort(cam0, R, p) then distort(cam1) (`cam1`: info of distort: atan_inverted, atan_interval)
      und1:  undistort(cam1, float32 guess)           (of `guess` when given: the device's own cam1 pixel)
    and `ref0`, `ref_guess`, `ref1`: the long-double results."""
    c = calib(pair, ext)
    (K0, D0, m0), (K1, D1, m1) = R.cams(c)
    if pts is None:
        pts = point_set(pair, ext)[0]
    i0, ig, i1 = {}, {}, {}
    ref0 = R.undistort(K0, D0, m0, pts, info=i0)
    ref_guess = R.stereo_guess(c, pts, info=ig)
    with np.errstate(over="ignore", invalid="ignore"):
        g32 = ref_guess.astype(np.float32) if guess is None else np.ascontiguousarray(guess, dtype=np.float32)
    ref1 = R.undistort(K1, D1, m1, g32, info=i1)
    return dict(und0=i0, guess=ig, und1=i1, ref0=ref0, ref_guess=ref_guess, ref1=ref1)


def branch_names(b):
    """The set of branch names reached by the points of one branches() record."""
    out = set()
    for stage in ("und0", "und1"):
        i = b[stage]
        if "steps" not in i:
            out.add("radtan")
            continue
        if i["floor"].any(): out.add("floor")
        if (~i["floor"] & (i["theta_d"] < 2e-8)).any(): out.add("over_floor")
        if i["clamp"].any(): out.add("clamp")
        if i["exhausted"].any(): out.add("exhausted")
        if (i["tan_inverted"] & ~i["floor"]).any(): out.add("tan_inverted")
        if (~i["tan_inverted"] & ~i["floor"]).any(): out.add("tan_direct")
        for s in np.unique(i["steps"][~i["floor"] & ~i["exhausted"]]):
            out.add("steps%d" % s)
    d = b["guess"]["cam1"]
    if "atan_interval" in d:
        for inv, iv in set(zip(d["atan_inverted"].tolist(), d["atan_interval"].tolist())):
            out.add("atan_%s%d" % ("inv" if inv else "dir", iv))
    return out


ALL_BRANCHES = ({"radtan", "floor", "over_floor", "clamp", "exhausted", "tan_inverted", "tan_direct", "steps1", "steps2",
                 "steps3", "steps4"} | {"atan_%s%d" % (s, i) for s in ("dir", "inv") for i in range(5)})


def judge(pair, ext, pts, out1, und0, und1):
    """The bars of the flat-image probe for one set, from the reference: `out1` (= the stereo guess), `und0`, `und1` as
    float32 n x 2.  Returns the figures and the list of violations (empty = the set passes).

    A coordinate of a well-conditioned point must be within 1 float32 ulp of the reference; at most ULP_CAP_SHARE of a
    stage's well-conditioned coordinates may differ from the rounded reference at all; at most ILL_CAP_SHARE of the points
    may be ill conditioned (those are held to the oracle only, and named); every output is finite.  und1 is judged against
    the reference's undistort of the guess that was handed in, so an earlier stage's last bit does not count twice."""
    b = branches(pair, ext, pts, guess=out1)
    well0 = np.asarray(b["und0"]["well"])
    stages = (("und0", und0, b["ref0"], well0), ("out1", out1, b["ref_guess"], well0),
              ("und1", und1, b["ref1"], np.asarray(b["und1"]["well"]) & np.isfinite(out1).all(1)))
    fig, bad = {}, []
    for name, got, ref, well in stages:
        got = np.ascontiguousarray(got, dtype=np.float32)
        if not np.isfinite(got).all():
            bad.append("%s: %d non-finite outputs, first at point %d" % (name, int((~np.isfinite(got)).any(1).sum()),
                                                                         int(np.argmax((~np.isfinite(got)).any(1)))))
        dist, margin = R.ulps32(got, ref)
        dw = dist[well]
        n_coord = dw.size
        n_off = int((dw != 0).sum())
        worst = int(dw.max()) if n_coord else 0
        ill = np.flatnonzero(~well)
        fig[name] = dict(worst_ulp=worst, off_by_one=n_off, coords=n_coord, ill=len(ill),
                         min_margin_of_off=float(margin[well][dw != 0].min()) if n_off else None)
        if worst > 1:
            i = int(np.argmax(np.where(well[:, None], dist, 0).max(1)))
            bad.append("%s: well-conditioned point %d %s is %d ulps from the reference" % (name, i, pts[i].tolist(), worst))
        if n_off > ULP_CAP_SHARE * n_coord:
            bad.append("%s: %d of %d coordinates differ from the rounded reference (cap %.1f %%)" % (name, n_off, n_coord, 100 * ULP_CAP_SHARE))
        if len(ill) > ILL_CAP_SHARE * len(pts):
            bad.append("%s: %d of %d points are ill conditioned (cap 2 %%)" % (name, len(ill), len(pts)))
        fig[name]["ill_points"] = ill.tolist()
    return fig, bad


def figures_line(pair, ext, fig):
    return "%s/%s: " % (pair, ext) + "; ".join("%s worst %d ulp, %d/%d off by one, %d ill" % (k, f["worst_ulp"], f["off_by_one"], f["coords"], f["ill"])
                                               for k, f in fig.items())


# ---------------------------------------------------------------------------------------------- det_atan / det_tan rings
def trig_ring_set(n_dirs=24):
    """The ideal lens pair (D = 0: theta_d = theta, Newton takes one step, und = tan(theta_d) (x, y) / theta_d and the guess
    is atan(r) (x, y) / r) under identity extrinsics, with only the rings that put det_tan's argument on each side of pi/4
    and towards pi/2, and det_atan's on each side of every reduction boundary, in n_dirs directions."""
    dirs = [(math.cos(a), math.sin(a)) for a in (2 * math.pi * (k + 0.31) / n_dirs for k in range(n_dirs))]
    c0 = CAMERAS["ideal0"]
    q, hp = math.pi / 4, math.pi / 2
    thetas = [q * (1 - 1e-2), q * (1 - 1e-5), q * (1 - 1e-7), q * (1 + 1e-7), q * (1 + 1e-5), q * (1 + 1e-2), 1.0, 1.3, 1.5,
              hp - 1e-2, hp - 1e-3, hp - 1e-4, hp - 1e-5, hp - 2e-6]
    pts = np.concatenate([_theta_pixels(c0, thetas, dirs), _cam1_ray_pixels("ideal", "identity", ATAN_RING_RADII, dirs)])
    assert len(pts) <= MAX_POINTS
    return pts


# ---------------------------------------------------------------------------------------------- the epipolar gate
GATE_SIZE = (129, 71)
GATE_RANKS = 12
GATE_MARGIN = 1e-9          # a point whose error lies within 1e-9 of the threshold (relative) is not judged
_G0 = _cam((78.0, 78.5, 64.2, 35.1), (-0.28, 0.07, 2e-4, 2e-5), RADTAN, GATE_SIZE)
_G1 = _cam((78.3, 77.9, 64.9, 35.4), (-0.27, 0.072, -1e-4, -3e-5), RADTAN, GATE_SIZE)
_SX, _SY = GATE_SIZE[0] / 752.0, GATE_SIZE[1] / 480.0
CAMERAS.update(
    gate0=_G0, gate1=_G1,
    gate_euroc0=_cam((458.654 * _SX, 457.296 * _SY, 367.215 * _SX, 248.375 * _SY), CAMERAS["euroc0"]["D"], RADTAN, GATE_SIZE),
    gate_euroc1=_cam((457.587 * _SX, 456.134 * _SY, 379.999 * _SX, 255.238 * _SY), CAMERAS["euroc1"]["D"], RADTAN, GATE_SIZE))
PAIRS.update(gate=("gate0", "gate1"), gate_euroc=("gate_euroc0", "gate_euroc1"))
# calibrations whose stereo guess lies within a few pixels of the point, so that on cam1 image = cam0 image the stereo LK
# converges back onto the point and status bit 1 is decided by the gate alone; the last has a vertical baseline (l0 dominates l1)
GATE_CASES = dict(identity=("gate", "identity"), euroc=("gate_euroc", "euroc"), verged05=("gate", "verged05"),
                  vertical=("gate", "vertical"))


def gate_inputs(name):
    """(calib, image, pts) of a gate case: the smooth canvas of the LK tests at 129 x 71 and a lattice of pitch 4."""
    import lk_cases
    w, h = GATE_SIZE
    img = lk_cases.crop(lk_cases.smooth_canvas(w, h, 4242), w, h)
    return calib(*GATE_CASES[name]), img, lk_cases.lattice(w, h, offset=0.37, pitch=4)


def gate_plan(c, und0, und1, matched):
    """From the undistorted points of the matched pairs: their long-double epipolar errors and GATE_RANKS values of
    stereo_threshold that put epi_thresh at the midpoint between two adjacent sorted errors, spread through the population
    (the middle one at the median)."""
    ex = R.extrinsics(c)
    err = R.epipolar_error(ex["E"], und0, und1)
    srt = np.sort(err[matched])
    unit = ex["epi_thresh"] / LD(5.0)
    n = len(srt)
    ranks = sorted(set([n // 2] + [int(round(1 + (n - 3) * k / (GATE_RANKS - 1))) for k in range(GATE_RANKS)]))
    thresholds = [float((srt[r - 1] + srt[r]) / 2 / unit) for r in ranks]
    return err, thresholds, float((srt[n // 2 - 1] + srt[n // 2]) / 2 / unit)


def gate_verdict(c, stereo_threshold, err, matched, accepted):
    """One threshold of the sweep: (number judged, number excluded by the margin, number accepted, indices that disagree)."""
    thr = R.extrinsics(c, stereo_threshold=stereo_threshold)["epi_thresh"]
    judged = matched & (np.abs(err - thr) > LD(GATE_MARGIN) * thr)
    want = err <= thr
    wrong = np.flatnonzero(judged & (want != accepted.astype(bool)))
    return int(judged.sum()), int((matched & ~judged).sum()), int((want & matched).sum()), wrong.tolist()
