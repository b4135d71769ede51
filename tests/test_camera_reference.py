"""The camera-geometry reference and case sets of tests/test_gpu_camera_geometry.py, on the CPU: the point sets reach every
branch they are meant to reach, the long-double reference is the model (round trips, a 40-digit evaluation) and notices
each of a list of deliberate mistakes, the CPU oracle (the device's operation sequence) stays within the GPU test's bars
on every set, its deterministic atan / tan hold their stated double-level accuracy, and the canvases of the epipolar-gate
sweep give the populations that test needs.  No GPU.

Figures observed (x86-64, 80-bit long double):
  * every set of FLAT_CASES: oracle = rounded reference on every well-conditioned coordinate (0 of 2318..2692 per stage
    differ), 0..22 ill-conditioned points per set (cap 2 %), no non-finite output;
  * radtan five-step residual over the sensor and its 10 % margin: euroc 0.79 / 1.19 px (cam0 / cam1), tang 6.8e-3 /
    9.7e-3 px, zero 1.4e-17 px (the rounding of the long doubles);
  * det_tan 4.5e-16, det_atan 4.1e-16 relative against tanl / atanl (bar 8 * 2^-53 = 8.9e-16);
  * long double against 40 digits, all 21 sets: at most 1.6e-18 (euroc/verged), scaled as
    test_long_double_reference_agrees_with_40_digits states; bar 1e-17;
  * mutations: each moves 0.02 % (pixel unit: the threshold itself) to 33 % of the well-conditioned outputs by 4 ulps or
    more; the Newton derivative 4, 6, 8 moves 92 outputs (only where the iteration runs out of its steps), the dropped
    float32 rounding 1.2 % (the largest by 5968 ulps).
"""
import numpy as np
import pytest

from msckf_stereo_c_amd.ctypes_types import default_fe_cfg

import camera_cases as C
import camera_reference as R
from camera_reference import EQUIDISTANT, LD

pytestmark = pytest.mark.skipif(not R.HAVE_LONG_DOUBLE, reason=R.NEED_LONG_DOUBLE)

CASE_IDS = ["%s-%s" % c for c in C.FLAT_CASES]
_BRANCHES = {}


def _branches(pair, ext):
    if (pair, ext) not in _BRANCHES:
        _BRANCHES[(pair, ext)] = C.branches(pair, ext)
    return _BRANCHES[(pair, ext)]


def _oracle_flat(oracle, pair, ext):
    """What the device returns for a set on a flat 64 x 64 pair, from the oracle: (guess, und0, und1, inliers)."""
    pts, _ = C.point_set(pair, ext)
    c = C.calib(pair, ext, 64, 64)
    flat = np.full((64, 64), 128, np.uint8)
    guess, m = oracle.stereo_match(c, default_fe_cfg(), flat, flat, pts)
    (K0, D0, m0), (K1, D1, m1) = R.cams(c)
    return guess, oracle.undistort(K0, D0, pts, model=m0), oracle.undistort(K1, D1, guess, model=m1), m


# ---------------------------------------------------------------------------------------------- the sets
def test_every_branch_is_reached():
    """Each atan interval on both sides of x = 1, tan direct and inverted, the 1e-8 floor from both sides, the clamp, Newton
    step counts 1 to 4 and the exhausted iteration occur in some set; every set fits one track call."""
    seen = set()
    for pair, ext in C.FLAT_CASES:
        pts, labels = C.point_set(pair, ext)
        assert len(pts) == len(labels) <= C.MAX_POINTS
        names = C.branch_names(_branches(pair, ext))
        print(pair, ext, len(pts), sorted(names))
        seen |= names
    assert not C.ALL_BRANCHES - seen, sorted(C.ALL_BRANCHES - seen)
    # the sides the ring pixels were chosen for are the sides the reference finds: both neighbours of every boundary
    b = _branches("ideal", "identity")
    labels = C.point_set("ideal", "identity")[1]
    ring = labels == "atan_rings"
    d = b["guess"]["cam1"]
    got = set(zip(np.asarray(d["atan_inverted"])[ring].tolist(), np.asarray(d["atan_interval"])[ring].tolist()))
    assert got == {(i, k) for i in (False, True) for k in range(5)}
    q = labels == "tan_quarter"
    assert b["und0"]["tan_inverted"][q].any() and (~b["und0"]["tan_inverted"][q]).any()
    rim = labels == "clamp_rim"
    assert b["und0"]["clamp"][rim].any() and (~b["und0"]["clamp"][rim]).any()
    # the last float32 pixel under the clamp and the first over it are neighbours
    fy, cy = C.CAMERAS["ideal0"]["K"][1], C.CAMERAS["ideal0"]["K"][3]
    v = C.point_set("ideal", "identity")[0][rim][:, 1]
    edge = np.float32(cy + fy * (np.pi / 2))
    assert edge in v and np.nextafter(edge, np.float32(0)) in v and np.nextafter(edge, np.float32(1e9)) in v


def test_floor_pairs_sit_on_both_sides_of_the_floor():
    for pair, want_floor in (("floor_under", True), ("floor_over", False)):
        pts, labels = C.point_set(pair, "identity")
        i = int(np.flatnonzero(labels == "principal")[0])
        info = _branches(pair, "identity")["und0"]
        assert bool(info["floor"][i]) == want_floor and 0.8e-8 < float(info["theta_d"][i]) < 1.2e-8


# ---------------------------------------------------------------------------------------------- the reference is the model
# five fixed-point steps are not the inverse: the residual |distort(undistort(p)) - p| is a property of the algorithm.  Bars:
# the value measured (docstring) with one decade of margin.
RADTAN_RESIDUAL_PX = dict(euroc0=8.0, euroc1=12.0, tang0=7e-2, tang1=1e-1, zero0=1e-15, zero1=1e-15)


def test_round_trip_through_the_forward_model():
    """distort is the closed-form model, undistort an iteration written from the published procedure: where Newton converges
    and the clamp is not hit they invert each other to 1e-9 px in long double; radtan's five steps leave a stated residual."""
    for name, cam in C.CAMERAS.items():
        rng = np.random.default_rng(7)
        parts = C._field(cam, rng)
        pts = np.concatenate([p for _, p in parts])
        info = {}
        und = R.undistort(cam["K"], cam["D"], cam["model"], pts, info=info)
        back = R.distort(cam["K"], cam["D"], cam["model"], und)           # long double in, taken as it is
        err = np.abs(back - pts.astype(LD)).max(1)
        if cam["model"] == EQUIDISTANT:
            ok = np.asarray(~info["clamp"] & ~info["exhausted"] & ~info["floor"])
            assert ok.sum() > 0.9 * len(pts)
            print("%s: round trip %.2e px over %d points" % (name, float(err[ok].max()), int(ok.sum())))
            assert float(err[ok].max()) < 1e-9
        elif name in RADTAN_RESIDUAL_PX:
            print("%s: five-step residual %.3e px" % (name, float(err.max())))
            assert float(err.max()) < RADTAN_RESIDUAL_PX[name]
    # all four coefficients zero: undistort is the identity map of the normalised coordinates
    cam = C.CAMERAS["zero0"]
    pts = C.point_set("zero", "roll90")[0]
    und = R.undistort(cam["K"], cam["D"], cam["model"], pts)
    fx, fy, cx, cy = (LD(v) for v in cam["K"])
    assert np.array_equal(und[:, 0], (pts[:, 0].astype(LD) - cx) / fx) and np.array_equal(und[:, 1], (pts[:, 1].astype(LD) - cy) / fy)


def _mp_undistort(mp, K, D, model, u, v, Rm):
    """40-digit restatement, one point; (x, y, scale of x, scale of y): what a relative error of the intermediate values
    is relative to in the result: the coordinate itself (radtan: the terms of its last difference, which are the
    coordinate unless the tangential part cancels it) times the amplification of the model (1 / the smallest denominator,
    tan's condition number), and after a rotation the terms of the row sums over W."""
    fx, fy, cx, cy = (mp.mpf(float(t)) for t in K)
    k = [mp.mpf(float(t)) for t in D]
    x, y = (mp.mpf(float(u)) - cx) / fx, (mp.mpf(float(v)) - cy) / fy
    amp = mp.mpf(1)
    if model == EQUIDISTANT:
        td = mp.sqrt(x * x + y * y)
        hp = mp.mpf(1.5707963267948966)
        if td > hp:
            td = hp
        scale = mp.mpf(0)
        if td > mp.mpf(1e-8):
            th = td
            for _ in range(10):
                t2 = th * th
                val = th * (1 + t2 * (k[0] + t2 * (k[1] + t2 * (k[2] + t2 * k[3]))))
                der = 1 + t2 * (3 * k[0] + t2 * (5 * k[1] + t2 * (7 * k[2] + t2 * 9 * k[3])))
                fix = (val - td) / der
                th -= fix
                amp = max(amp, 1 / abs(der))
                if abs(fix) < mp.mpf(1e-8):
                    break
            scale = mp.tan(th) / td
            amp = max(amp, abs(th / (mp.sin(th) * mp.cos(th))))          # the condition number of tan
        x, y = x * scale, y * scale
    else:
        k1, k2, p1, p2 = k
        x0, y0 = x, y
        for _ in range(5):
            r2 = x * x + y * y
            den = 1 + (k2 * r2 + k1) * r2
            dx, dy = 2 * p1 * x * y + p2 * (r2 + 2 * x * x), p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
            x, y = (x0 - dx) / den, (y0 - dy) / den
            amp = max(amp, 1 / abs(den))
            tx, ty = (abs(x0) + abs(dx)) / abs(den), (abs(y0) + abs(dy)) / abs(den)      # the terms of the last difference
    sx, sy = (abs(x) * amp, abs(y) * amp) if model == EQUIDISTANT else (tx * amp, ty * amp)
    if Rm is not None:
        X = Rm[0][0] * x + Rm[0][1] * y + Rm[0][2]
        Y = Rm[1][0] * x + Rm[1][1] * y + Rm[1][2]
        W = Rm[2][0] * x + Rm[2][1] * y + Rm[2][2]
        # every entry of R is a sum of three products of entries <= 1 (three units), every row sum takes (x, y) with their
        # own scale: X / W carries row(X) / |W| + |X| row(W) / W^2
        row = 3 * (abs(x) + abs(y) + 1) + sx + sy
        sx, sy = row / abs(W) + abs(X) * row / (W * W), row / abs(W) + abs(Y) * row / (W * W)
        x, y = X / W, Y / W
    return x, y, sx, sy


def _mp_distort(mp, K, D, model, xf, yf):
    """(u, v, scale of u, scale of v): the scales are |fx xd| + |cx|, what a relative error of the terms is relative to."""
    fx, fy, cx, cy = (mp.mpf(float(t)) for t in K)
    k = [mp.mpf(float(t)) for t in D]
    x, y = mp.mpf(float(xf)), mp.mpf(float(yf))
    if model == EQUIDISTANT:
        r = mp.sqrt(x * x + y * y)
        th = mp.atan(r)
        t2 = th * th
        thd = th * (1 + t2 * (k[0] + t2 * (k[1] + t2 * (k[2] + t2 * k[3]))))
        s = thd / r if r > mp.mpf(1e-8) else mp.mpf(1)
        xd, yd = x * s, y * s
    else:
        k1, k2, p1, p2 = k
        r2 = x * x + y * y
        cd = 1 + r2 * (k1 + k2 * r2)
        xd = x * cd + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
        yd = y * cd + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
    return xd * fx + cx, yd * fy + cy, abs(xd * fx) + abs(cx), abs(yd * fy) + abs(cy)


def _mp_extrinsic_R(mp, c):
    T0 = [[mp.mpf(float(c.T_cam0_imu[4 * i + j])) for j in range(4)] for i in range(4)]
    T10 = [[mp.mpf(float(c.T_cam1_cam0[4 * i + j])) for j in range(4)] for i in range(4)]
    R0 = mp.matrix([r[:3] for r in T0[:3]])
    R1 = mp.matrix([r[:3] for r in T10[:3]]) * R0
    # R_cam0_imu = R0^T, R_cam1_imu = R1^T, R_cam0_cam1 = R_cam1_imu^T R_cam0_imu
    M = R1 * R0.T
    return [[M[i, j] for j in range(3)] for i in range(3)]


@pytest.mark.parametrize("pair,ext", C.FLAT_CASES, ids=CASE_IDS)
def test_long_double_reference_agrees_with_40_digits(pair, ext):
    """Every set of FLAT_CASES through an mpmath restatement with true tan / atan at 40 digits.  The bar is 1e-17 relative,
    where `relative` has to say to what: the 64-bit long double carries 1.1e-19 per operation, and a result that comes out
    of a cancellation or a division by a small number carries that error relative to the operands, not to itself.  So an
    undistorted coordinate is held to 1e-17 of itself times the amplification the 40-digit evaluation itself reports
    (1 / the smallest denominator, tan's condition number theta / (sin cos), each at least 1), a rotated one to 1e-17 of
    its row sums' terms over W (a row sum that cancels leaves values near 1e-20 that no relative bar of their own fits),
    a pixel to 1e-17 (|f xd| + |c|)."""
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 40
    pts, labels = C.point_set(pair, ext)
    c = C.calib(pair, ext)
    (K0, D0, m0), (K1, D1, m1) = R.cams(c)
    Rm = _mp_extrinsic_R(mp, c)
    b = _branches(pair, ext)
    with np.errstate(over="ignore", invalid="ignore"):
        mid = b["guess"]["und"].astype(np.float32)
        g32 = b["ref_guess"].astype(np.float32)
    worst = 0.0
    tol = mp.mpf("1e-17")
    # a Newton iteration that runs out of its ten steps without settling multiplies a difference at every step, by no
    # simple figure: those points are left to the other tests (bit for bit against the oracle, float32 against this reference)
    skip0 = np.asarray(b["und0"].get("exhausted", np.zeros(len(pts), bool)))
    skip1 = np.asarray(b["und1"].get("exhausted", np.zeros(len(pts), bool)))

    def held(ref_ld, x, y, sx, sy, what, i):
        nonlocal worst
        for got, want, scale in ((ref_ld[0], x, sx), (ref_ld[1], y, sy)):
            if not np.isfinite(got):
                continue
            hi = float(got)                                     # a long double is the sum of two doubles, exactly
            g = mp.mpf(hi) + mp.mpf(float(got - LD(hi)))
            e = abs(g - want) / scale if scale else abs(g - want)
            worst = max(worst, float(e))
            assert e <= tol, (what, i, pts[i].tolist(), float(e))

    for i in range(len(pts)):
        if not skip0[i]:
            held(b["ref0"][i], *_mp_undistort(mp, K0, D0, m0, pts[i, 0], pts[i, 1], None), "und0", i)
            held(b["guess"]["und"][i], *_mp_undistort(mp, K0, D0, m0, pts[i, 0], pts[i, 1], Rm), "rotated", i)
        if np.isfinite(mid[i]).all():
            held(b["ref_guess"][i], *_mp_distort(mp, K1, D1, m1, mid[i, 0], mid[i, 1]), "guess", i)
        if np.isfinite(g32[i]).all() and not skip1[i]:
            held(b["ref1"][i], *_mp_undistort(mp, K1, D1, m1, g32[i, 0], g32[i, 1], None), "und1", i)
    print("%s/%s: %d points, worst scaled difference %.2e" % (pair, ext, len(pts), worst))


# ---------------------------------------------------------------------------------------------- the oracle within the bars
@pytest.mark.parametrize("pair,ext", C.FLAT_CASES, ids=CASE_IDS)
def test_oracle_stays_within_the_bars_of_the_gpu_test(oracle, pair, ext):
    """The CPU preview of tests/test_gpu_camera_geometry.py: the oracle's stereo guess on a flat pair (LK returns it
    unchanged, status 0) and its undistorted points against the reference, by the same judge and the same caps."""
    pts, labels = C.point_set(pair, ext)
    guess, und0, und1, inl = _oracle_flat(oracle, pair, ext)
    assert not inl.any()
    fig, bad = C.judge(pair, ext, pts, guess, und0, und1)
    print(C.figures_line(pair, ext, fig))
    for k, f in fig.items():
        if f["ill_points"]:
            print("  %s ill conditioned: %s" % (k, ", ".join("%s %s" % (labels[i], pts[i].tolist()) for i in f["ill_points"])))
    assert not bad, bad
    assert np.isfinite(guess).all() and np.isfinite(und0).all() and np.isfinite(und1).all()


def test_ideal_lens_rim_is_finite(oracle):
    """The pixels whose theta_d clamps to the double pi/2, where a one-part reduction pi/2 - t is exactly zero: finite
    outputs, and tan at the clamp is 1 / (the low part of pi/2)."""
    K, D = [140.0, 140.0, 320.0, 240.0], [0.0] * 4
    pts = np.array([(320, 465), (321, 465), (550, 240), (320, 15), (90, 240)], np.float32)
    und = oracle.undistort(K, D, pts, model=1)
    assert np.isfinite(und).all()
    t = oracle.det_trig("tan", [1.5707963267948966])[0]
    assert abs(t * 6.123233995736766e-17 - 1.0) < 1e-15
    assert und[0, 0] == 0.0 and abs(float(und[0, 1]) / (225.0 / 140.0 * t / 1.5707963267948966) - 1.0) < 1e-7


# ---------------------------------------------------------------------------------------------- det_atan / det_tan as doubles
TRIG_BAR = 8 * 2.0 ** -53       # 8.9e-16, see the test


def test_deterministic_trig_double_accuracy(oracle):
    """det_tan on (0, pi/2] and det_atan on (0, 1e300) as doubles against tanl / atanl.  The bar is eight units of 2^-53
    relative, from the operation count: tan is a quotient of two Horner sums (each result within about two units: the
    rounding of t^2 enters damped, the last multiply-add and the product with t undamped), a division (one) and, above
    pi/4, the reduction, which after the two-part constant is exact up to one rounding of the reduced argument, amplified
    by tan's condition number t / (sin t cos t) <= pi/2 there (one and a half units); atan has the rounded constant atan(c),
    the quotient z with three roundings scaled by z p / atan <= 1, the final sum, and for x > 1 the reciprocal and the
    subtraction from pi/2.  Dense sweeps, both sides of every reduction boundary, the approach to pi/2 down to the clamp."""
    hp = 1.5707963267948966
    rng = np.random.default_rng(1)
    t = np.concatenate([np.linspace(0, hp, 400001)[1:], hp - np.logspace(-17, -1, 2000), np.pi / 4 + np.linspace(-1e-6, 1e-6, 2001),
                        rng.uniform(0, hp, 200000), np.logspace(-300, -1, 3000), [hp, np.nextafter(hp, 0)]])
    t = t[(t > 0) & (t <= hp)]
    got = oracle.det_trig("tan", t)
    ref = np.tan(t.astype(LD))
    rel = np.abs((got.astype(LD) - ref) / ref).astype(np.float64)
    print("det_tan: worst %.3e at %.17g; above pi/4 %.3e; within 1e-6 of pi/2 %.3e" %
          (rel.max(), t[rel.argmax()], rel[t > np.pi / 4].max(), rel[t > hp - 1e-6].max()))
    assert np.isfinite(got).all() and rel.max() < TRIG_BAR
    x = np.concatenate([np.logspace(-300, 300, 100001), np.linspace(0, 2, 400001)[1:], rng.uniform(0, 1, 200000),
                        1 / rng.uniform(1e-3, 1, 100000)] +
                       [b + np.linspace(-1e-6, 1e-6, 401) for b in (0.125, 0.375, 0.625, 0.875, 1, 1 / 0.875, 1 / 0.625, 1 / 0.375, 8)])
    got = oracle.det_trig("atan", x)
    ref = np.arctan(x.astype(LD))
    rel = np.abs((got.astype(LD) - ref) / ref).astype(np.float64)
    print("det_atan: worst %.3e at %.17g; x > 1 %.3e" % (rel.max(), x[rel.argmax()], rel[x > 1].max()))
    assert rel.max() < TRIG_BAR


# ---------------------------------------------------------------------------------------------- the reference notices mistakes
def _stage_outputs(pair, ext, mutate):
    """und0, the stereo guess, und1 (of the unmutated float32 guess) and the epipolar error of (und0, und1), long double."""
    c = C.calib(pair, ext)
    (K0, D0, m0), (K1, D1, m1) = R.cams(c)
    pts = C.point_set(pair, ext)[0]
    base = _branches(pair, ext)
    with np.errstate(over="ignore", invalid="ignore"):
        g32 = base["ref_guess"].astype(np.float32)
        u0, u1 = base["ref0"].astype(np.float32), base["ref1"].astype(np.float32)
    ex = R.extrinsics(c, mutate=mutate)
    with np.errstate(all="ignore"):
        epi = R.epipolar_error(ex["E"], u0, u1)
    return dict(und0=R.undistort(K0, D0, m0, pts, mutate=mutate), guess=R.stereo_guess(c, pts, mutate=mutate),
                und1=R.undistort(K1, D1, m1, g32, mutate=mutate), epi=np.stack([epi, epi], 1),
                thresh=np.full((1, 2), ex["epi_thresh"]))


_RIGHT = {}


def _well(pair, ext):
    b = _branches(pair, ext)
    w0 = np.asarray(b["und0"]["well"])
    w1 = np.asarray(b["und1"]["well"]) & w0
    return dict(und0=w0, guess=w0, und1=w1, epi=w1, thresh=np.ones(1, bool))


@pytest.mark.parametrize("mutation", R.MUTATIONS)
def test_reference_notices_the_mistake(mutation):
    """Each deliberate mistake moves at least one well-conditioned output of some set by 4 float32 ulps or more (the dropped
    float32 rounding between the two halves of the stereo guess is half an ulp of the ray: it shows where the pixel
    f xd + c is small against its terms).  A reference that could not tell these apart from the contract would let a
    kernel with the same mistake pass."""
    moved = total = 0
    worst, where = 0, None
    for pair, ext in C.FLAT_CASES:
        right = _RIGHT.setdefault((pair, ext), _stage_outputs(pair, ext, None))
        wrong = _stage_outputs(pair, ext, mutation)
        well = _well(pair, ext)
        for k in right:
            with np.errstate(over="ignore", invalid="ignore"):
                r32 = right[k].astype(np.float32)
            fin = np.isfinite(r32).all(1) & well[k]
            dist, _ = R.ulps32(r32, wrong[k])
            d = dist[fin].max(1) if fin.any() else np.zeros(0, np.int64)
            moved += int((d >= 4).sum())
            total += int(fin.sum())
            if len(d) and d.max() > worst:
                worst, where = int(d.max()), (pair, ext, k)
    print("%s: %d of %d well-conditioned outputs move (%.2f %%), the largest by %d ulps at %s" %
          (mutation, moved, total, 100.0 * moved / total, worst, where))
    assert moved >= 1 and worst >= 4


def test_ulps32_counts_and_margins():
    one = np.float32(1.0)
    up = np.nextafter(one, np.float32(2))
    tie = (LD(one) + LD(up)) / 2
    d, m = R.ulps32(np.array([one, up, one, np.float32(0), np.float32(-0.0), np.float32(np.nan)]),
                    np.array([LD(one), LD(one), tie + LD(1e-12), LD(0), LD(0), LD(1)]))
    assert d.tolist()[:5] == [0, 1, 1, 0, 0] and d[5] >= 2 ** 31
    assert m[0] == 0.5 and m[2] < 1e-4
    d, _ = R.ulps32(np.array([np.float32(-1e-45)]), np.array([LD(1e-45)]))
    assert d[0] == 2


# ---------------------------------------------------------------------------------------------- the epipolar gate's inputs
@pytest.mark.parametrize("name", sorted(C.GATE_CASES))
def test_gate_canvases_give_the_populations(oracle, name):
    """The conditions of the gate sweep, on the oracle: at least 200 matched points, the match back on the point (so bit 1
    is the gate's alone), a quarter of them on each side of the median threshold, at most 1 % lost to the margin, the
    oracle's verdict = the reference's at every threshold, and nothing but the verdict moving with the threshold."""
    c, img, pts = C.gate_inputs(name)
    fe = default_fe_cfg()
    fe.stereo_threshold = 1e9
    (K0, D0, m0), (K1, D1, m1) = R.cams(c)
    out1, inl = oracle.stereo_match(c, fe, img, img, pts)
    matched = inl.astype(bool)
    und0, und1 = oracle.undistort(K0, D0, pts, model=m0), oracle.undistort(K1, D1, out1, model=m1)
    assert matched.sum() >= 200 and np.abs(out1 - pts)[matched].max() < 0.05
    err, thresholds, median = C.gate_plan(c, und0, und1, matched)
    assert len(thresholds) >= C.GATE_RANKS and median in thresholds
    E = np.asarray(R.extrinsics(c)["E"], dtype=np.float64)
    l = E @ np.array([0.1, 0.1, 1.0])
    assert (abs(l[0]) > 10 * abs(l[1])) == (name == "vertical")
    for thr in thresholds:
        fe.stereo_threshold = thr
        o1, acc = oracle.stereo_match(c, fe, img, img, pts)
        assert np.array_equal(o1.view(np.uint32), out1.view(np.uint32))
        judged, excluded, n_acc, wrong = C.gate_verdict(c, thr, err, matched, acc)
        assert not wrong, (name, thr, wrong)
        assert excluded <= 0.01 * matched.sum()
        assert not acc[~matched].any()
        if thr == median:
            assert n_acc >= matched.sum() // 4 and matched.sum() - n_acc >= matched.sum() // 4
