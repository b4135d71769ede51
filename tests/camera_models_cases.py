"""Lenses, extrinsics and point sets of the opt-in camera-model tests (tests/test_camera_models_reference.py on the CPU,
tests/test_gpu_camera_models.py on the device), the bars of the flat-pair probe, and the fit of fov / ds parameters to the
synthetic rig's radtan lens for the Runner tests.

The values are the test author's choice:
  cv5       EuRoC's intrinsics and k1 k2 p1 p2 with an OpenCV-style fifth coefficient k3 = 0.0121 / 0.0117 (752 x 480; positive, so that the
            lens stays monotone out to the sensor's corners as EuRoC's own does);
  rational  a CALIB_RATIONAL_MODEL wide lens, fx = 380.8 at 752 x 480, eight coefficients;
  fov       w = 0.93 / 0.95 on TUM-VI-like intrinsics (512 x 512, fx = 190.98): rd w reaches pi/2 at 322 px from the principal
            point, inside the corners (362 px), so corner pixels are outside the domain by construction;
  ds        TUM-VI-like: 512 x 512, fx = 172.98 / 173.44, xi = -0.21 / -0.19, alpha = 0.59 / 0.61: 90 degrees off axis lies about
            334 px from the principal point, so corner pixels are outside the domain (ray z <= 0) by construction, and the 10 %
            margin around the sensor reaches r2 > 1 / (2 alpha - 1) (408 px).
The extrinsics are those of tests/camera_cases.py.
"""
import numpy as np

import camera_cases as CC
import camera_models_reference as M
import camera_reference as R

LD = R.LD
ULP_CAP_SHARE, ILL_CAP_SHARE = CC.ULP_CAP_SHARE, CC.ILL_CAP_SHARE      # the existing test's bars, as they are
COUNTS = (0, 1, 3, 4, 5, 63, 64, 257)


def _cam(K, model, coeffs, size):
    return dict(K=tuple(float(v) for v in K), model=model, coeffs=tuple(float(v) for v in coeffs), size=size)


E0, E1 = CC.CAMERAS["euroc0"], CC.CAMERAS["euroc1"]
CAMERAS = dict(
    cv5_0=_cam(E0["K"], M.RADTAN8, E0["D"] + (0.0121,), (752, 480)),
    cv5_1=_cam(E1["K"], M.RADTAN8, E1["D"] + (0.0117,), (752, 480)),
    rational0=_cam((380.8, 380.7, 365.8, 254.3), M.RADTAN8, (0.4532, 0.0876, 0.00042, -0.00031, 0.0019, 0.7841, 0.2103, 0.0112), (752, 480)),
    rational1=_cam((379.9, 380.2, 370.1, 250.6), M.RADTAN8, (0.4498, 0.0851, -0.00037, 0.00029, 0.0021, 0.7795, 0.2071, 0.0118), (752, 480)),
    fov0=_cam((190.98, 190.97, 254.93, 256.90), M.FOV, (0.93,), (512, 512)),
    fov1=_cam((190.44, 190.43, 252.59, 254.91), M.FOV, (0.95,), (512, 512)),
    ds0=_cam((172.98, 172.97, 254.93, 256.90), M.DS, (-0.21, 0.59), (512, 512)),
    ds1=_cam((173.44, 173.43, 252.59, 254.91), M.DS, (-0.19, 0.61), (512, 512)),
    # base models, as a stream on an extended model may have one on its other camera
    radtan1=_cam(E1["K"], M.RADTAN, E1["D"], (752, 480)),
    equi0=_cam(CC.CAMERAS["mild0"]["K"], M.EQUIDISTANT, CC.CAMERAS["mild0"]["D"], (752, 480)),
)
# name -> (cam0, cam1, extrinsics of camera_cases)
CASES = dict(
    cv5=("cv5_0", "cv5_1", "euroc"),
    rational=("rational0", "rational1", "verged"),
    fov=("fov0", "fov1", "identity"),
    ds=("ds0", "ds1", "euroc"),
    ds_verged=("ds0", "ds1", "verged"),
    fov_ds=("fov0", "ds1", "verged"),
    cv5_radtan=("cv5_0", "radtan1", "identity"),
    equi_rational=("equi0", "rational1", "euroc"),
)
CASE_NAMES = sorted(CASES)


def cams(case):
    c0, c1, _ = CASES[case]
    return CAMERAS[c0], CAMERAS[c1]


def calib(case, width=64, height=64):
    """The mskf_calib of a case: a camera on an extended model gets fx fy cx cy and a zero radtan (the setter brings the model)."""
    from msckf_stereo_c_amd.ctypes_types import Calib
    c0, c1 = cams(case)
    c = Calib()
    c.width, c.height = width, height
    for i in range(4):
        c.cam0_intrinsics[i], c.cam1_intrinsics[i] = c0["K"][i], c1["K"][i]
        c.cam0_distortion[i] = c0["coeffs"][i] if c0["model"] < M.RADTAN8 else 0.0
        c.cam1_distortion[i] = c1["coeffs"][i] if c1["model"] < M.RADTAN8 else 0.0
    c.cam0_model = c0["model"] if c0["model"] < M.RADTAN8 else M.RADTAN
    c.cam1_model = c1["model"] if c1["model"] < M.RADTAN8 else M.RADTAN
    T0, T10 = CC.EXTRINSICS[CASES[case][2]]
    for i in range(16):
        c.T_cam0_imu[i], c.T_cam1_cam0[i] = T0.flat[i], T10.flat[i]
        c.T_imu_body[i] = np.eye(4).flat[i]
    return c


def apply_models(stream, case):
    """Set the case's extended models on a capi.Stream (base-model cameras are left to the calibration)."""
    for i, cam in enumerate(cams(case)):
        if cam["model"] >= M.RADTAN8:
            stream.set_camera_model(i, M.MODEL_NAMES[cam["model"]], cam["coeffs"])


def R01_64(case):
    """R_cam0_cam1 as mskf_stream_create computes it, in float64 (host_math.h: plain products in this order)."""
    T0 = np.asarray(CC.EXTRINSICS[CASES[case][2]][0], np.float64)
    T10 = np.asarray(CC.EXTRINSICS[CASES[case][2]][1], np.float64)
    return _r01(T0, T10)


def _mat3(a, b):
    """3 x 3 product with the sums in index order (a[i][0] b[0][j] + a[i][1] b[1][j] + a[i][2] b[2][j]), as a plain C loop has it."""
    out = np.zeros((3, 3))
    for i in range(3):
        for j in range(3):
            s = 0.0
            for k in range(3):
                s = s + a[i, k] * b[k, j]
            out[i, j] = s
    return out


def _r01(T0, T10):
    R_cam0_imu = T0[:3, :3].T.copy()
    R1 = _mat3(T10[:3, :3], T0[:3, :3])
    R_cam1_imu = R1.T.copy()
    return _mat3(R_cam1_imu.T.copy(), R_cam0_imu)


_SETS = {}


def point_set(case):
    """float32 pixels (n x 2) of a case: a grid and a seeded cloud over cam0's sensor with a 10 % margin around it (rim pixels,
    and for fov / ds the pixels outside the domain), the sensor's corners and edge midpoints, the principal point (exactly, when
    float32 holds it; the nearest pixels otherwise) and its row and column."""
    if case not in _SETS:
        c0, _ = cams(case)
        w, h = c0["size"]
        rng = np.random.default_rng(sum(map(ord, case)))
        x0, x1, y0, y1 = -0.1 * w, (w - 1) + 0.1 * w, -0.1 * h, (h - 1) + 0.1 * h
        gx, gy = np.meshgrid(np.linspace(x0, x1, 21), np.linspace(y0, y1, 17))
        cloud = np.stack([rng.uniform(x0, x1, 380), rng.uniform(y0, y1, 380)], 1)
        cx, cy = c0["K"][2], c0["K"][3]
        rim = [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1), (w // 2, 0), (w // 2, h - 1), (0, h // 2), (w - 1, h // 2)]
        centre = [(cx, cy), (np.floor(cx), np.floor(cy)), (np.ceil(cx), np.ceil(cy))] + [(cx, v) for v in np.linspace(0, h - 1, 9)] + [(u, cy) for u in np.linspace(0, w - 1, 9)]
        pts = np.concatenate([np.stack([gx.ravel(), gy.ravel()], 1), cloud, np.array(rim, float), np.array(centre, float)]).astype(np.float32)
        pts.setflags(write=False)
        _SETS[case] = pts
    return _SETS[case]


def expected(case, pts):
    """The float64 restatement's flat-pair result for a case."""
    c0, c1 = cams(case)
    return M.track_flat64((c0["K"], c0["model"], c0["coeffs"]), (c1["K"], c1["model"], c1["coeffs"]), R01_64(case), pts)


def judge(case, pts, out1, und0, und1):
    """The bars of the flat-pair probe against the long-double model (those of camera_cases.judge, taken over as they are): every
    well-conditioned coordinate within 1 float32 ulp, at most ULP_CAP_SHARE of them off the rounded reference at all, at most
    ILL_CAP_SHARE of a set's points ill conditioned (camera_models_reference's rule); a point outside the domain must be (0, 0).
    und1 is judged against the model's undistortion of the out1 handed in.  Returns (figures, violations)."""
    c0, c1 = cams(case)
    T0, T10 = CC.EXTRINSICS[CASES[case][2]]

    class _C:
        T_cam0_imu, T_cam1_cam0 = T0.ravel(), T10.ravel()
        cam0_intrinsics, cam1_intrinsics = c0["K"], c1["K"]
    R01 = R.extrinsics(_C)["R"]
    i0, ir, ig, i1 = {}, {}, {}, {}
    ref0, ok0 = M.undistort_ld(c0["K"], c0["model"], c0["coeffs"], pts, info=i0)
    ray, okr = M.undistort_ld(c0["K"], c0["model"], c0["coeffs"], pts, Rm=R01, info=ir)
    with np.errstate(all="ignore"):
        mid = np.where(okr[:, None], ray, LD(0)).astype(np.float32)
    refg, okg = M.distort_ld(c1["K"], c1["model"], c1["coeffs"], mid, info=ig)
    okg = okg & okr
    out1 = np.ascontiguousarray(out1, np.float32)
    ref1, ok1 = M.undistort_ld(c1["K"], c1["model"], c1["coeffs"], out1, info=i1)
    stages = (("und0", und0, ref0, ok0, i0["well"]), ("out1", out1, refg, okg, ir["well"] & (ig["well"] | ~okr)), ("und1", und1, ref1, ok1, i1["well"]))
    fig, bad = {}, []
    for name, got, ref, ok, well in stages:
        got = np.ascontiguousarray(got, np.float32)
        well = np.asarray(well, bool)
        if not np.isfinite(got).all():
            bad.append("%s: non-finite outputs" % name)
        outside = well & ~ok
        if (got[outside] != 0).any():
            bad.append("%s: a point outside the domain is not (0, 0)" % name)
        sel = well & ok
        dist, _ = R.ulps32(got, np.where(ok[:, None], ref, LD(0)))
        dw = dist[sel]
        n_off, worst = int((dw != 0).sum()), int(dw.max()) if dw.size else 0
        ill = int((~well).sum())
        fig[name] = dict(worst_ulp=worst, off_by_one=n_off, coords=int(dw.size), ill=ill, outside=int(outside.sum()))
        if worst > 1:
            i = int(np.argmax(np.where(sel[:, None], dist, 0).max(1)))
            bad.append("%s: well-conditioned point %d %s is %d ulps from the reference" % (name, i, pts[i].tolist(), worst))
        if n_off > ULP_CAP_SHARE * dw.size:
            bad.append("%s: %d of %d coordinates differ from the rounded reference (cap 0.1 %%)" % (name, n_off, dw.size))
        if ill > ILL_CAP_SHARE * len(pts):
            bad.append("%s: %d of %d points are ill conditioned (cap 2 %%)" % (name, ill, len(pts)))
    return fig, bad


def figures_line(case, fig):
    return "%s: " % case + "; ".join("%s worst %d ulp, %d/%d off by one, %d ill, %d outside" % (k, f["worst_ulp"], f["off_by_one"], f["coords"], f["ill"], f["outside"])
                                     for k, f in fig.items())


# ------------------------------------------------------------------------------------------ fov / ds fitted to a radtan lens
def fit_to_radtan(K, D, size, model, steps=60):
    """Parameters of `model` (M.FOV: [w]; M.DS: [xi, alpha]) and the focal scale s that best reproduce, in pixels, the radtan
    lens (K, D) over the image: both models magnify the image centre (fov by 2 tan(w / 2) / w, ds by 1 / (1 + xi)), which a
    calibration absorbs in its focal lengths, so the fitted camera is K' = (s fx, s fy, cx, cy) with the model's parameters.
    Damped, reweighted Gauss-Newton with a forward-difference Jacobian on the residuals distort_model(K', ray) - pixel over a 24 x 16 grid of pixels
    (ray = the radtan lens's converged undistortion of the pixel).  Returns (parameters, K', largest residual in pixels)."""
    w, h = size
    gx, gy = np.meshgrid(np.linspace(0, w - 1, 24), np.linspace(0, h - 1, 16))
    px = np.stack([gx.ravel(), gy.ravel()], 1).astype(np.float32)
    rays = M.exact_undistort_ld(K, M.RADTAN8, list(D) + [0.0] * 4, px)

    def k_of(p):
        return (float(p[-1]) * K[0], float(p[-1]) * K[1], K[2], K[3])

    def resid(p):
        out, ok = M.distort_ld(k_of(p), model, [float(v) for v in p[:-1]], rays)
        return (out - px.astype(LD)).astype(np.float64).ravel() if ok.all() else None

    def valid(p):
        return (0.05 < p[0] < 3.0) if model == M.FOV else (-0.9 < p[0] <= 1.0 and 0.0 <= p[1] <= 1.0)
    p = np.array([0.9, 0.93] if model == M.FOV else [-0.2, 0.6, 0.8])
    for _ in range(steps):
        r = resid(p)
        # the bar is on the LARGEST residual: each step weighs a pixel by (its residual / the largest)^3, which pulls the least-squares
        # answer towards the minimax one
        n = np.sqrt((r.reshape(-1, 2) ** 2).sum(1))
        wt = np.repeat((n / n.max()) ** 3 + 1e-3, 2)
        J = np.stack([(resid(p + np.eye(len(p))[i] * 1e-6) - r) / 1e-6 for i in range(len(p))], 1)
        step = 0.5 * np.linalg.lstsq(J * wt[:, None], r * wt, rcond=None)[0]
        for _ in range(20):          # halve the step until it stays in the model's domain
            q = p - step
            if valid(q) and resid(q) is not None:
                p = q
                break
            step = step / 2
    p = np.array([float(np.float32(v)) for v in p])          # short, exactly representable values
    r = resid(p).reshape(-1, 2)
    return p[:-1].tolist(), k_of(p), float(np.sqrt((r * r).sum(1)).max())
