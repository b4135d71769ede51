"""The opt-in camera models on the CPU ("Extended camera models"): csrc/hip/fe_cam_models.h compiled with g++
against the float64 restatement of tests/camera_models_reference.py bit for bit, the restatement against the long-double model
(and that against mpmath), the degenerate radtan8 against the oracle's radtan, round trips, the domain edges, the deliberate
mistakes, the camchain reader and the fov / ds parameters the Runner tests use.  tests/test_gpu_camera_models.py runs the same
cases on the device.

Observed (x86-64): header == restatement on all 8 cases, both directions, R and identity; the restatement alone against the
long-double model: 0 ulp worst, 0 coordinates off, at most 2 ill-conditioned points of a set of 766 (cap 2 % = 15), 118 .. 135 points
outside the domain on the fov / ds cases; within the sensor radtan8's five steps leave 0.076 px on the cv5 lens and 13.2 px in the
corners of the rational lens, measured through the forward model (the procedure, not the exact inverse, is the contract); fov / ds
round trips within 6e-17 px; every mutation moves more than a thousand well-conditioned outputs by 4 ulps or more; the lenses
fitted to the rig leave 2.0 / 2.8 px (fov) and 1.2 / 1.3 px (ds) against the gate's 5.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import camera_cases as CC
import camera_models_cases as MC
import camera_models_reference as M
import camera_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = R.LD
needs_ld = pytest.mark.skipif(not R.HAVE_LONG_DOUBLE, reason=R.NEED_LONG_DOUBLE)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a.view(np.uint64) if a.dtype == np.float64 else a


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _dp(a):
    return np.ascontiguousarray(a, np.float64).ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def hdr(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("fe_cam_models") / "libfe_cam_models_test.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-shared", "-fPIC", "-I", ROOT, "-o", so,
                           os.path.join(ROOT, "tests", "cpp", "fe_cam_models_test.cpp")])
    L = C.CDLL(so)
    L.fcm_det_atan.restype = L.fcm_det_tan.restype = C.c_double
    L.fcm_det_atan.argtypes = L.fcm_det_tan.argtypes = [C.c_double]

    class H:
        lib = L

        @staticmethod
        def undistort(K, model, coeffs, px, Rm=None):
            px = np.ascontiguousarray(px, np.float32).reshape(-1, 2)
            out, ok = np.zeros_like(px), np.zeros(len(px), np.uint8)
            k = np.array(M.coeffs8(model, coeffs))
            r = None if Rm is None else np.ascontiguousarray(Rm, np.float64).reshape(9)
            L.fcm_undistort_points(len(px), _dp(K), model, _dp(k), None if r is None else r.ctypes.data_as(C.c_void_p), px.ctypes.data_as(C.c_void_p),
                                   out.ctypes.data_as(C.c_void_p), ok.ctypes.data_as(C.c_void_p))
            return out, ok.astype(bool)

        @staticmethod
        def distort(K, model, coeffs, xy):
            xy = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
            out, ok = np.zeros_like(xy), np.zeros(len(xy), np.uint8)
            k = np.array(M.coeffs8(model, coeffs))
            L.fcm_distort_points(len(xy), _dp(K), model, _dp(k), xy.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), ok.ctypes.data_as(C.c_void_p))
            return out, ok.astype(bool)

        @staticmethod
        def undistort_norm(model, coeffs, x, y):
            xy = np.array([x, y], np.float64)
            ok = L.fcm_undistort_norm(model, _dp(np.array(M.coeffs8(model, coeffs))), xy.ctypes.data_as(C.c_void_p))
            return bool(ok), xy

        @staticmethod
        def distort_norm(model, coeffs, x, y):
            xy, out = np.array([x, y], np.float64), np.zeros(2)
            ok = L.fcm_distort_norm(model, _dp(np.array(M.coeffs8(model, coeffs))), xy.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
            return bool(ok), out
    return H


# ------------------------------------------------------------------------------------------ header == restatement
def test_det_trig_restated(hdr):
    x = np.concatenate([np.linspace(0, 1.2, 4001), [0.125, 0.375, 0.625, 0.875, 1.0, 1e-300, 3.0, 1e9]])
    assert _same(M.det_atan64(x), np.array([hdr.lib.fcm_det_atan(float(v)) for v in x]))
    t = np.concatenate([np.linspace(0, 1.5707963267948966, 4001), [0.78539816339744830962, 1e-300]])
    assert _same(M.det_tan64(t), np.array([hdr.lib.fcm_det_tan(float(v)) for v in t]))


@pytest.mark.parametrize("case", MC.CASE_NAMES)
def test_header_equals_the_restatement(hdr, case):
    """Every extended camera of a case: undistort through R and through the identity path, distort of the rotated rays, bit for
    bit with the in-domain flags, on the points the GPU test uses."""
    pts = MC.point_set(case)
    c0, c1 = MC.cams(case)
    R01 = MC.R01_64(case)
    exp = MC.expected(case, pts)
    n_out = 0
    for cam, px in ((c0, pts), (c1, exp["out1"])):
        if cam["model"] < M.RADTAN8:
            continue
        for Rm in (None, R01):
            got, ok = hdr.undistort(cam["K"], cam["model"], cam["coeffs"], px, Rm)
            want, wok = M.undistort64(cam["K"], cam["model"], cam["coeffs"], px, Rm)
            assert np.array_equal(ok, wok) and _same(got, want), (case, Rm is None)
            n_out += int((~ok).sum())
    ray, _ = M.undistort64(c0["K"], c0["model"], c0["coeffs"], pts, R01)
    if c1["model"] >= M.RADTAN8:
        got, ok = hdr.distort(c1["K"], c1["model"], c1["coeffs"], ray)
        want, wok = M.distort64(c1["K"], c1["model"], c1["coeffs"], ray)
        assert np.array_equal(ok, wok) and _same(got, want), case
    if case in ("fov", "ds", "ds_verged", "fov_ds"):
        assert n_out > 0          # points outside the domain by construction


def test_restated_base_models_equal_the_oracle(oracle):
    """The restatement's radtan and equidistant (a mixed stream's base camera) are the oracle's, bit for bit, both directions."""
    for pair, ext in (("euroc", "euroc"), ("tumvi", "roll90"), ("kalibr", "vertical"), ("tang", "vertical")):
        pts = CC.point_set(pair, ext)[0]
        c = CC.calib(pair, ext)
        (K0, D0, m0), (K1, D1, m1) = R.cams(c)
        Rm = np.asarray(R.extrinsics(c)["R"], np.float64)
        assert _same(M.undistort64(K0, m0, D0, pts)[0], oracle.undistort(K0, D0, pts, model=m0))
        ray = oracle.undistort(K0, D0, pts, R=Rm, model=m0)
        assert _same(M.undistort64(K0, m0, D0, pts, Rm)[0], ray)
        assert _same(M.distort64(K1, m1, D1, ray)[0], oracle.distort(K1, D1, ray, model=m1))


def test_degenerate_radtan8_is_radtan(hdr, oracle):
    """radtan8 with k3 .. k6 = 0 gives the bits of the oracle's radtan, both directions, header and restatement."""
    for pair, ext in (("euroc", "euroc"), ("tang", "vertical"), ("zero", "roll90")):
        pts = CC.point_set(pair, ext)[0]
        c = CC.calib(pair, ext)
        (K0, D0, _), (K1, D1, _) = R.cams(c)
        Rm = np.asarray(R.extrinsics(c)["R"], np.float64)
        for K, D in ((K0, D0), (K1, D1)):
            for r in (None, Rm):
                want = oracle.undistort(K, D, pts, R=r, model=0)
                assert _same(hdr.undistort(K, M.RADTAN8, list(D) + [0.0] * 4, pts, r)[0], want)
                assert _same(M.undistort64(K, M.RADTAN8, list(D) + [0.0] * 4, pts, r)[0], want)
        ray = oracle.undistort(K0, D0, pts, R=Rm, model=0)
        want = oracle.distort(K1, D1, ray, model=0)
        assert _same(hdr.distort(K1, M.RADTAN8, list(D1) + [0.0] * 4, ray)[0], want)
        assert _same(M.distort64(K1, M.RADTAN8, list(D1) + [0.0] * 4, ray)[0], want)


# ------------------------------------------------------------------------------------------ restatement against the long-double model
@needs_ld
@pytest.mark.parametrize("case", MC.CASE_NAMES)
def test_restatement_stays_within_the_bars_of_the_gpu_test(case):
    """What the device must equal bit for bit passes the GPU test's bars against the long-double model on its own, and the
    ill-conditioned points stay under the cap."""
    pts = MC.point_set(case)
    exp = MC.expected(case, pts)
    fig, bad = MC.judge(case, pts, exp["out1"], exp["und0"], exp["und1"])
    print(MC.figures_line(case, fig))
    assert not bad, bad
    assert all(f["coords"] > 0.5 * len(pts) for f in fig.values())


@needs_ld
def test_long_double_model_agrees_with_mpmath():
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 40
    f = mp.mpf
    xs = [(0.3, -0.2), (1.1, 0.7), (-0.05, 0.02)]
    # fov
    w = f(0.93)
    for x, y in xs:
        ru = mp.sqrt(f(x) ** 2 + f(y) ** 2)
        s = mp.atan(2 * ru * mp.tan(w / 2)) / w / ru
        got, _ = M.distort_ld((1, 1, 0, 0), M.FOV, (0.93,), np.array([[x, y]], LD))
        assert abs(f(float(got[0, 0])) - f(x) * s) < 1e-17 * 10 and abs(f(float(got[0, 1])) - f(y) * s) < 1e-17 * 10
    # ds, the paper's projection
    xi, al = f(-0.21), f(0.59)
    for x, y in xs:
        r2 = f(x) ** 2 + f(y) ** 2
        d1 = mp.sqrt(r2 + 1)
        d2 = mp.sqrt(r2 + (xi * d1 + 1) ** 2)
        den = al * d2 + (1 - al) * (xi * d1 + 1)
        got, _ = M.distort_ld((1, 1, 0, 0), M.DS, (-0.21, 0.59), np.array([[x, y]], LD))
        # (float(longdouble) keeps 53 bits: compare at double precision, the constants -0.21 / 0.59 being doubles on both sides)
        assert abs(f(float(got[0, 0])) - f(x) / den) < 1e-15 and abs(f(float(got[0, 1])) - f(y) / den) < 1e-15


@needs_ld
def test_round_trip():
    """distort(undistort(p)) = p within 1e-9 px for fov and ds on in-domain pixels (closed-form inverses); radtan8's five steps are
    the published procedure: what they leave against the converged inverse is reported."""
    worst = {}
    for name in ("fov0", "fov1", "ds0", "ds1"):
        cam = MC.CAMERAS[name]
        pts = MC.point_set({"fov0": "fov", "fov1": "fov", "ds0": "ds", "ds1": "ds"}[name])
        info = {}
        und, ok = M.undistort_ld(cam["K"], cam["model"], cam["coeffs"], pts, info=info)
        sel = ok & info["well"]
        back, ok2 = M.distort_ld(cam["K"], cam["model"], cam["coeffs"], und[sel])
        assert ok2.all() and sel.sum() > 300
        err = np.abs(back - pts[sel].astype(LD)).max()
        worst[name] = float(err)
        assert err < 1e-9, (name, float(err))
    for name, case in (("cv5_0", "cv5"), ("rational0", "rational")):
        cam = MC.CAMERAS[name]
        pts = MC.point_set(case)
        pts = pts[(pts[:, 0] >= 0) & (pts[:, 0] <= cam["size"][0] - 1) & (pts[:, 1] >= 0) & (pts[:, 1] <= cam["size"][1] - 1)]     # the sensor: the iteration converges there
        five, _ = M.undistort_ld(cam["K"], cam["model"], cam["coeffs"], pts)
        back, _ = M.distort_ld(cam["K"], cam["model"], cam["coeffs"], five)
        worst[name] = float(np.abs(back - pts.astype(LD)).max())          # what the five steps leave, through the forward model
    print("round trips (px): %s" % worst)


# ------------------------------------------------------------------------------------------ domain edges
def test_domain_edges(hdr):
    up, dn = (lambda v: float(np.nextafter(v, np.inf))), (lambda v: float(np.nextafter(v, -np.inf)))
    # ds: r2 = 1 / (2 alpha - 1) and one ulp either side.  At that edge mz = -(1 - alpha)^2 / ((2 alpha - 1)(1 - alpha)) < 0: the
    # ray already points backwards, so on the z = 1 plane the z rule refuses every point the r2 rule lets through there.  What
    # the r2 rule decides, and that the ray it lets through is a finite number (1 - (2 alpha - 1) r2 may round below 0), shows
    # on the ray itself.  alpha = 0.625: 2 alpha - 1 = 0.25, the edge is r2 = 4 exactly; alpha = 0.59 / 0.61: a rounded edge.
    def ray(ds, mx, my):
        out = np.zeros(3)
        ok = hdr.lib.fcm_ds_ray_norm(_dp(np.array(M.coeffs8(M.DS, ds))), _dp(np.array([mx, my])), out.ctypes.data_as(C.c_void_p))
        return bool(ok), out
    n_at_edge = 0
    for ds in ((-0.2, 0.625), (-0.21, 0.59), (-0.19, 0.61), (0.5, 1.0)):
        edge = 1.0 / (2.0 * ds[1] - 1.0)
        for r2, inside in ((edge, True), (dn(edge), True), (up(edge), False)):
            hit = None          # a normalised pixel whose mx * mx + my * my is r2 exactly, as the header forms it
            for mx in np.linspace(0.25, 1.0, 61):
                my0 = float(np.sqrt(r2 - mx * mx))
                for my in (my0, dn(my0), up(my0), dn(dn(my0)), up(up(my0))):
                    if float(mx) * float(mx) + my * my == r2:
                        hit = (float(mx), my)
                        break
                if hit:
                    break
            assert hit, (ds, r2)
            ok, v = ray(ds, *hit)
            assert ok == inside, (ds, r2)
            if inside and ds[1] < 1.0:
                assert np.isfinite(v).all() and v[2] <= 0.0 and not hdr.undistort_norm(M.DS, ds, *hit)[0]
            if inside and ds[1] == 1.0:          # alpha = 1: 0 / 0 at the edge itself; what is no number is outside the domain
                assert not hdr.undistort_norm(M.DS, ds, *hit)[0]
            n_at_edge += 1
    assert n_at_edge == 12
    ds = (-0.2, 0.625)
    # ds ray z at 0 from both sides: bisect the radius where t mz - xi changes sign
    lo, hi = 0.1, 2.0
    assert hdr.undistort_norm(M.DS, ds, lo, 0.0)[0] and not hdr.undistort_norm(M.DS, ds, hi, 0.0)[0]
    while up(lo) < hi:
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if hdr.undistort_norm(M.DS, ds, mid, 0.0)[0] else (lo, mid)
    ok, xy = hdr.undistort_norm(M.DS, ds, lo, 0.0)
    assert ok and np.isfinite(xy).all() and xy[0] > 1e3          # the last ray in front of the camera: finite, far out
    assert not hdr.undistort_norm(M.DS, ds, hi, 0.0)[0]
    # ds projection: z = 1 rays are always in the paper's domain for these parameters; a negative denominator is refused
    assert hdr.distort_norm(M.DS, ds, 50.0, -20.0)[0]
    assert not hdr.distort_norm(M.DS, (-0.999, 0.0), 1e3, 0.0)[0]          # den = xi d1 + 1 < 0
    # fov: rd w = pi/2 and one ulp below (w = 1: rd w is rd itself)
    ok, _ = hdr.undistort_norm(M.FOV, (1.0,), M.HALF_PI, 0.0)
    assert not ok
    ok, xy = hdr.undistort_norm(M.FOV, (1.0,), dn(M.HALF_PI), 0.0)
    assert ok and np.isfinite(xy).all() and xy[0] > 1e15
    # the 1e-8 floors from both sides: the limit below, the quotient at and above; both finite and within 1e-15 of each other
    for w in (0.93, 1.0):
        lim_u, lim_d = w / (2 * np.tan(w / 2)), 2 * np.tan(w / 2) / w
        for r in (dn(1e-8), 1e-8, up(1e-8), 0.0):
            ok, xy = hdr.undistort_norm(M.FOV, (w,), r, 0.0)
            assert ok and np.isfinite(xy).all() and (r == 0.0 or abs(xy[0] / r - lim_u) < 1e-7)
            ok, out = hdr.distort_norm(M.FOV, (w,), r, 0.0)
            assert ok and np.isfinite(out).all() and (r == 0.0 or abs(out[0] / r - lim_d) < 1e-7)
        below, at = hdr.undistort_norm(M.FOV, (w,), dn(1e-8), 0.0)[1][0] / dn(1e-8), hdr.undistort_norm(M.FOV, (w,), 1e-8, 0.0)[1][0] / 1e-8
        assert below == pytest.approx(lim_u, rel=1e-15) and at == pytest.approx(lim_u, rel=1e-8)
    # the setter's coefficient check
    v = hdr.lib.fcm_validate_model
    k = lambda *a: _dp(np.array(list(a) + [0.0] * (8 - len(a))))
    assert v(M.FOV, k(0.93)) == 0 and v(M.FOV, k(0.0)) == 3 and v(M.FOV, k(np.pi)) == 3 and v(M.FOV, k(dn(np.pi))) == 0
    assert v(M.DS, k(-1.0, 0.5)) == 4 and v(M.DS, k(1.0, 0.5)) == 0 and v(M.DS, k(up(1.0), 0.5)) == 4
    assert v(M.DS, k(0.0, -1e-9)) == 5 and v(M.DS, k(0.0, 0.0)) == 0 and v(M.DS, k(0.0, 1.0)) == 0 and v(M.DS, k(0.0, up(1.0))) == 5
    assert v(5, k()) == 1 and v(-1, k()) == 1 and v(M.RADTAN8, k(np.nan)) == 2 and v(M.RADTAN, k(0, 0, 0, 0, 0, 0, 0, np.inf)) == 2


# ------------------------------------------------------------------------------------------ mutations
@needs_ld
@pytest.mark.parametrize("mutation", M.MUTATIONS)
def test_reference_notices_the_mistake(mutation):
    """Each deliberate mistake moves some well-conditioned output of the model it concerns by at least 4 float32 ulps."""
    model = M.MUTATION_MODEL[mutation]
    worst = moved = 0
    for name, cam in MC.CAMERAS.items():
        if cam["model"] != model:
            continue
        case = [c for c in MC.CASE_NAMES if MC.CASES[c][0] == name or MC.CASES[c][1] == name][0]
        pts = MC.point_set(case)
        info = {}
        right, ok = M.undistort_ld(cam["K"], model, cam["coeffs"], pts, info=info)
        wrong, ok2 = M.undistort_ld(cam["K"], model, cam["coeffs"], pts, mutate=mutation)
        sel = ok & ok2 & info["well"]
        d = R.ulps32(right[sel].astype(np.float32), wrong[sel])[0]
        rays = right[sel].astype(np.float32)
        pr, okp = M.distort_ld(cam["K"], model, cam["coeffs"], rays)
        pw, okw = M.distort_ld(cam["K"], model, cam["coeffs"], rays, mutate=mutation)
        both = okp & okw
        d2 = R.ulps32(pr[both].astype(np.float32), pw[both])[0]
        for dd in (d, d2):
            if dd.size:
                worst = max(worst, int(dd.max()))
                moved += int((dd.max(1) >= 4).sum())
    print("%s: %d well-conditioned outputs move by 4 ulps or more, the largest by %d" % (mutation, moved, worst))
    assert moved >= 1 and worst >= 4


# ------------------------------------------------------------------------------------------ the camchain reader
_CAMCHAIN = """cam0:
  T_cam_imu:
    [0.0148655429818, -0.999880929698, 0.00414029679422, -0.0216401454975,
     0.999557249008, 0.0149672133247, 0.025715529948, -0.064676986768,
     -0.0257744366974, 0.00375618835797, 0.999660727178, 0.00981073058949,
     0.0, 0.0, 0.0, 1.0]
%s
  resolution: [752, 480]
cam1:
  T_cn_cnm1:
    [0.999997256478, 0.00231206719242, 0.000376008102415, -0.110073808127,
     -0.00231713572328, 0.999898048507, 0.0140898358466, 0.000399121547014,
     -0.000343393120525, -0.0140906685727, 0.999900662638, -0.000853702503357,
     0.0, 0.0, 0.0, 1.0]
%s
  resolution: [752, 480]
T_imu_body:
  [1.0000, 0.0000, 0.0000, 0.0000,
  0.0000, 1.0000, 0.0000, 0.0000,
  0.0000, 0.0000, 1.0000, 0.0000,
  0.0000, 0.0000, 0.0000, 1.0000]
"""
_PIN = "  camera_model: pinhole\n  distortion_coeffs: %s\n  distortion_model: %s\n  intrinsics: [458.654, 457.296, 367.215, 248.375]"
_DS = "  camera_model: ds\n  intrinsics: [-0.21, 0.59, 172.98, 172.97, 254.93, 256.90]%s"


def _load(tmp_path, name, cam0, cam1):
    from msckf_stereo_c_amd import build
    from msckf_stereo_c_amd.ctypes_types import Calib, EkfCfg, FeCameraModel, FeCfg
    import shutil
    build.build_all()
    L = C.CDLL(os.path.join(ROOT, "msckf_stereo_c_amd", "_build", "libmskf_host.so"))
    d = tmp_path / name
    shutil.copytree(os.path.join(ROOT, "config"), d)
    (d / "camchain-imucam-euroc.yaml").write_text(_CAMCHAIN % (cam0, cam1))
    models, ext = (FeCameraModel * 2)(), (C.c_int * 2)()
    rc_m = L.mskfh_load_camera_models(str(d / "camchain-imucam-euroc.yaml").encode(), models, ext)
    calib, fe, ekf = Calib(), FeCfg(), EkfCfg()
    rc_c = L.mskfh_load_configs(str(d).encode(), C.byref(calib), C.byref(fe), C.byref(ekf))
    return rc_m, rc_c, models, list(ext), calib


def test_camchain_forms(tmp_path, oracle):
    four, five = "[-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05]", "[-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05, -0.0121]"
    eight = "[0.4532, 0.0876, 0.00042, -0.00031, 0.0019, 0.7841, 0.2103, 0.0112]"
    # four coefficients: today's path, bit for bit
    rc_m, rc_c, m, ext, calib = _load(tmp_path, "four", _PIN % (four, "radtan"), _PIN % (four, "equidistant"))
    ref = oracle.euroc_calib(752, 480)
    assert (rc_m, rc_c, ext) == (0, 0, [0, 0]) and (calib.cam0_model, calib.cam1_model) == (0, 1)
    assert list(calib.cam0_distortion) == list(ref.cam0_distortion) and list(calib.cam0_intrinsics) == list(ref.cam0_intrinsics)
    assert (m[0].cam, m[0].model, m[1].cam, m[1].model) == (0, 0, 1, 1) and list(m[0].coeffs)[:4] == list(ref.cam0_distortion)
    # five padded with zeros, eight as they are; cam1 fov
    rc_m, rc_c, m, ext, calib = _load(tmp_path, "five", _PIN % (five, "radtan"), _PIN % ("[0.93]", "fov"))
    assert (rc_m, rc_c, ext) == (0, 0, [1, 1]) and (m[0].model, m[1].model) == (M.RADTAN8, M.FOV)
    assert list(m[0].coeffs) == [-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05, -0.0121, 0.0, 0.0, 0.0]
    assert list(m[1].coeffs) == [0.93] + [0.0] * 7 and (calib.cam0_model, calib.cam1_model) == (0, 0)
    assert list(calib.cam1_intrinsics) == [458.654, 457.296, 367.215, 248.375] and list(calib.cam1_distortion) == [0.0] * 4
    rc_m, rc_c, m, ext, calib = _load(tmp_path, "eight", _PIN % (eight, "radtan"), _DS % "")
    assert (rc_m, rc_c, ext) == (0, 0, [1, 1]) and (m[0].model, m[1].model) == (M.RADTAN8, M.DS)
    assert list(m[0].coeffs) == [0.4532, 0.0876, 0.00042, -0.00031, 0.0019, 0.7841, 0.2103, 0.0112]
    assert list(m[1].coeffs)[:2] == [-0.21, 0.59] and list(calib.cam1_intrinsics) == [172.98, 172.97, 254.93, 256.90]
    # Kalibr writes the absent distortion out
    rc_m, rc_c, m, ext, _ = _load(tmp_path, "ds_none", _DS % "\n  distortion_model: none\n  distortion_coeffs: []", _DS % "\n  distortion_model: none")
    assert (rc_m, rc_c, ext) == (0, 0, [1, 1]) and m[0].model == m[1].model == M.DS
    # refused
    bad = [(_PIN % ("[0.1, 0.2, 0.3]", "radtan"), "three radtan"), (_PIN % ("[0.1, 0.2, 0.3, 0.4, 0.5, 0.6]", "radtan"), "six radtan"),
           (_PIN % (five, "equidistant"), "five equidistant"), (_PIN % ("[0.9, 0.1]", "fov"), "two fov"), (_PIN % (four, "fov"), "four fov"),
           (_PIN % (four, "thinprism"), "unknown distortion"), ((_PIN % (four, "radtan")).replace("pinhole", "omni"), "omni"),
           (_DS % "\n  distortion_model: radtan\n  distortion_coeffs: %s" % four, "ds with distortion"),
           ("  camera_model: ds\n  intrinsics: [172.98, 172.97, 254.93, 256.90]", "ds with four intrinsics"),
           ("  camera_model: pinhole\n  distortion_coeffs: %s\n  distortion_model: radtan\n  intrinsics: [-0.21, 0.59, 172.98, 172.97, 254.93, 256.90]" % four, "pinhole with six")]
    for i, (cam, what) in enumerate(bad):
        rc_m, rc_c, _, _, _ = _load(tmp_path, "bad%d" % i, cam, _PIN % (four, "radtan"))
        assert rc_m == -1 and rc_c == -1, what
        rc_m, rc_c, _, _, _ = _load(tmp_path, "bad%db" % i, _PIN % (four, "radtan"), cam)
        assert rc_m == -1 and rc_c == -1, what


# ------------------------------------------------------------------------------------------ the Runner tests' fitted lenses
@needs_ld
def test_fitted_fov_and_ds_stay_under_the_epipolar_gate(oracle):
    """fov / ds parameters (and the focal scale that goes with them) fitted to the synthetic rig's radtan lens at the small test
    size: the largest residual over the image, in pixels, printed and held under the rig's epipolar-gate threshold
    (stereo_threshold = 5 px in the normalised unit 4 / (fx0 + fy0 + fx1 + fy1)), the condition under which the GPU run keeps
    its stereo matches: the two cameras have nearly the same lens, so the residuals of a match's two pixels point the same way
    and the epipolar distance moves by less than either."""
    from msckf_stereo_c_amd.ctypes_types import default_fe_cfg
    w, h = 188, 120
    calib = oracle.euroc_calib(w, h)
    for model in (M.FOV, M.DS):
        for K, D in ((list(calib.cam0_intrinsics), list(calib.cam0_distortion)), (list(calib.cam1_intrinsics), list(calib.cam1_distortion))):
            p, Kf, res = MC.fit_to_radtan(K, D, (w, h), model)
            print("%s fitted to the rig's radtan lens at %d x %d: %s with fx, fy = %.3f, %.3f (the rig's %.3f, %.3f), largest residual %.4f px"
                  % (M.MODEL_NAMES[model], w, h, p, Kf[0], Kf[1], K[0], K[1], res))
            assert res < default_fe_cfg().stereo_threshold
            assert len(p) == (1 if model == M.FOV else 2)
