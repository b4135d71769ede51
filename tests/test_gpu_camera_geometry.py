"""The per-point camera geometry of k_track4 (undistort_pt, distort_pt, the stereo guess through R_cam0_cam1, the epipolar
gate) against the plain long-double reference of tests/camera_reference.py, on the calibrations and point sets of
tests/camera_cases.py, and bit for bit against the CPU oracle on the same inputs.

  * Flat-image probe: on a constant 64 x 64 stereo pair no pyramid level can be solved, so mskf_fe_track returns the stereo
    guess itself in out1 (moved down and up the pyramid by powers of two, which is exact), status 1, out0 = the input,
    und0 = undistort(cam0, p), und1 = undistort(cam1, guess).  Points outside the 64 x 64 image take the idle slot of the
    level gates (lk_cases' border sets drive that path on real images).  Every well-conditioned coordinate must be within
    one float32 ulp of the reference, at most 0.1 % of a set's coordinates may differ from the rounded reference at all,
    at most 2 % of a set's points may be ill conditioned (camera_reference's rule; those are held to the oracle only),
    and nothing may be NaN or infinite.
  * det_atan / det_tan through the ideal lens (D = 0), ring by ring around every reduction boundary.
  * The epipolar gate: thresholds placed between adjacent sorted long-double errors of the device's own und0 / und1.
  * mskf_fe_track_batch over streams of different calibrations and models.

tests/test_camera_reference.py shows on the CPU that the sets reach their branches, that the reference notices a list of
deliberate mistakes, and that the oracle alone stays within the same bars.

Observed on MI355X (28 tests, under a second together):
  * flat probe, all 21 (pair, extrinsics) cases: out1, und0, und1 and status equal the oracle bit for bit; against the
    reference the worst well-conditioned coordinate is 0 ulp away and 0 of 2318..2692 coordinates per stage and set differ
    from the rounded reference (cap 0.1 %); no non-finite output.  Ill-conditioned points (held to the oracle only):
    ideal 22 of 1346 (und0, out1; und1 22 under identity extrinsics, 0 verged), floor_under / floor_over 20 of 1342,
    tumvi 17 of 1338 (und1 0..2), kalibr 1 of 1338, every other set 0: the image corners of the lenses whose image circle
    lies inside the sensor, the clamp_rim and theta_rim subsets within 1e-6 rad of pi/2 and beyond it, and the three
    ideal_rim_clamped pixels (cap 2 % = 26 of 1338).
  * ideal lens rim: und0 of (320, 465) = (0, 1.6709127e16), of (550, 240) = (1.7080441e16, 0): finite.
  * det_atan / det_tan rings (1200 points, 24 directions): 0 ulp, 0 of 2400 differ in each of und0, out1, und1; no
    ill-conditioned point.
  * gate: 507 of 527 points matched in each of the four cases, 13 thresholds each, 0 points excluded by the 1e-9 margin,
    no wrong verdict; errors 2.8e-2..5.3e-2 (euroc), 1.5e-6..2.0e-2 (identity), 9.1e-5..2.6e-2 (verged05), 3.2e-5..5.4e-2
    (vertical); the error closest to a threshold lay 9.4e-6 of it away (relative).
"""
import numpy as np
import pytest

from msckf_stereo_c_amd import capi
from msckf_stereo_c_amd.ctypes_types import default_ekf_cfg, default_fe_cfg

import camera_cases as C
import camera_reference as R

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not R.HAVE_LONG_DOUBLE, reason=R.NEED_LONG_DOUBLE)]

FIELDS = ("out0", "out1", "und0", "und1", "status")
FLAT = np.full((64, 64), 128, np.uint8)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32) if a.dtype == np.float32 else a


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _flat_track(gpu_ctx, c, pts):
    s = capi.Stream(gpu_ctx, c, default_fe_cfg(), default_ekf_cfg())
    s.push_stereo(FLAT, FLAT)
    got = s.track(pts, do_temporal=False)
    s.close()
    return got


def _check_flat(got, oracle, pair, ext, c, pts, labels=None):
    """One flat-pair result against the oracle (bits) and the reference (the bars of camera_cases.judge)."""
    (K0, D0, m0), (K1, D1, m1) = R.cams(c)
    assert (got["status"] == 1).all()
    assert _same(got["out0"], pts)
    guess, inl = oracle.stereo_match(c, default_fe_cfg(), FLAT, FLAT, pts)
    assert not inl.any()
    assert _same(got["out1"], guess)
    assert _same(got["und0"], oracle.undistort(K0, D0, pts, model=m0))
    assert _same(got["und1"], oracle.undistort(K1, D1, guess, model=m1))
    fig, bad = C.judge(pair, ext, pts, got["out1"], got["und0"], got["und1"])
    print(C.figures_line(pair, ext, fig))
    if labels is not None:
        for k, f in fig.items():
            if f["ill_points"]:
                print("  %s ill conditioned: %s" % (k, ", ".join("%s %s" % (labels[i], pts[i].tolist()) for i in f["ill_points"])))
    assert not bad, bad
    for k in ("out1", "und0", "und1"):
        assert np.isfinite(got[k]).all(), k
    return fig


@pytest.mark.parametrize("pair,ext", C.FLAT_CASES, ids=["%s-%s" % c for c in C.FLAT_CASES])
def test_flat_pair_probe_against_the_reference(gpu_ctx, oracle, pair, ext):
    pts, labels = C.point_set(pair, ext)
    c = C.calib(pair, ext, 64, 64)
    _check_flat(_flat_track(gpu_ctx, c, pts), oracle, pair, ext, c, pts, labels)


def test_ideal_lens_rim_pixels_are_finite(gpu_ctx, oracle):
    """The pixels whose theta_d clamps to the double pi/2, where a one-part reduction pi/2 - t is exactly zero: finite
    und0, guess and und1, equal to the oracle's."""
    c = C.calib("ideal", "identity", 64, 64)
    pts = np.array([(320, 465), (321, 465), (550, 240), (320, 15), (90, 240), (320, 240)], np.float32)
    got = _flat_track(gpu_ctx, c, pts)
    (K0, D0, m0), _ = R.cams(c)
    for k in ("out1", "und0", "und1"):
        assert np.isfinite(got[k]).all(), (k, got[k])
    assert (got["status"] == 1).all()
    assert _same(got["und0"], oracle.undistort(K0, D0, pts, model=m0))
    assert got["und0"][0, 0] == 0.0 and 1.6e16 < got["und0"][0, 1] < 1.7e16       # (225 / 140) tan(pi/2 as a double) / (pi/2)
    print("ideal lens rim: und0 %s" % got["und0"][:3].tolist())


def test_det_trig_rings_through_the_ideal_lens(gpu_ctx, oracle):
    """D = 0: und0 = tan(theta_d) (x, y) / theta_d and the guess is atan(r) (x, y) / r, so the float32 outputs hold
    det_tan / det_atan against tanl / atanl: 24 directions of rings on each side of pi/4, towards pi/2, and on each side of
    every reduction boundary of atan (x and 1 / x at 0.125, 0.375, 0.625, 0.875, 1)."""
    pts = C.trig_ring_set()
    c = C.calib("ideal", "identity", 64, 64)
    got = _flat_track(gpu_ctx, c, pts)
    fig = _check_flat(got, oracle, "ideal", "identity", c, pts)
    b = C.branches("ideal", "identity", pts, guess=got["out1"])
    d = b["guess"]["cam1"]
    assert set(zip(np.asarray(d["atan_inverted"]).tolist(), np.asarray(d["atan_interval"]).tolist())) == {(i, k) for i in (False, True) for k in range(5)}
    assert b["und0"]["tan_inverted"].any() and (~b["und0"]["tan_inverted"]).any()
    assert all(f["ill"] == 0 for f in fig.values())


@pytest.mark.parametrize("name", sorted(C.GATE_CASES))
def test_epipolar_gate_at_its_threshold(gpu_ctx, oracle, name):
    """cam1 image = cam0 image and a calibration whose guess lies beside the point: the stereo LK converges back onto the
    point and status bit 1 is the gate's alone.  The device's own und0 / und1 of a first call (huge threshold) give the
    long-double errors; streams whose stereo_threshold puts epi_thresh midway between adjacent sorted errors must accept
    exactly the points at or under it (a point within 1e-9 of the threshold, relative, is not judged), and nothing but
    bit 1 may move with the threshold."""
    c, img, pts = C.gate_inputs(name)

    def run(stereo_threshold):
        fe = default_fe_cfg()
        fe.stereo_threshold = stereo_threshold
        s = capi.Stream(gpu_ctx, c, fe, default_ekf_cfg())
        s.push_stereo(img, img)
        got = s.track(pts, do_temporal=False)
        s.close()
        return got

    base = run(1e9)
    matched = (base["status"] >> 1 & 1).astype(bool)
    assert (base["status"] & 1).all() and matched.sum() >= 200
    assert np.abs(base["out1"] - pts)[matched].max() < 0.05
    fe = default_fe_cfg()
    fe.stereo_threshold = 1e9
    ref_c1, ref_in = oracle.stereo_match(c, fe, img, img, pts)
    assert _same(base["out1"], ref_c1) and np.array_equal(matched, ref_in.astype(bool))
    err, thresholds, median = C.gate_plan(c, base["und0"], base["und1"], matched)
    assert len(thresholds) >= C.GATE_RANKS and median in thresholds
    worst_excluded = 0
    closest = np.inf
    for thr in thresholds:
        got = run(thr)
        for k in ("out0", "out1", "und0", "und1"):
            assert _same(got[k], base[k]), (name, thr, k)
        assert (got["status"] & 1).all()
        acc = got["status"] >> 1 & 1
        assert not acc[~matched].any()
        judged, excluded, n_acc, wrong = C.gate_verdict(c, thr, err, matched, acc)
        assert not wrong, (name, thr, wrong, [float(err[i]) for i in wrong])
        assert excluded <= 0.01 * matched.sum()
        worst_excluded = max(worst_excluded, excluded)
        t = R.extrinsics(c, stereo_threshold=thr)["epi_thresh"]
        closest = min(closest, float((np.abs(err[matched] - t) / t).min()))
        if thr == median:
            assert n_acc >= matched.sum() // 4 and matched.sum() - n_acc >= matched.sum() // 4
    print("gate %s: %d matched of %d, %d thresholds, errors %.2e..%.2e, at most %d excluded by the margin, closest error to a "
          "threshold %.1e relative" % (name, int(matched.sum()), len(pts), len(thresholds), float(err[matched].min()),
                                       float(err[matched].max()), worst_excluded, closest))


def test_track_batch_of_mixed_calibrations(gpu_ctx, oracle):
    """One mskf_fe_track_batch over four streams of different calibrations, models and extrinsics: every stream gets the
    bits it gets alone (the per-stream CamDev / R01 / E records must not leak between the blocks of a launch)."""
    cases = [("euroc", "euroc"), ("tumvi", "roll90"), ("radtan_equi", "verged"), ("equi_radtan", "euroc")]
    streams, kw, alone = [], [], []
    for pair, ext in cases:
        c = C.calib(pair, ext, 64, 64)
        pts = np.ascontiguousarray(C.point_set(pair, ext)[0])
        s = capi.Stream(gpu_ctx, c, default_fe_cfg(), default_ekf_cfg())
        s.push_stereo(FLAT, FLAT)
        streams.append(s)
        kw.append(dict(pts=pts, do_temporal=False))
        alone.append(s.track(pts, do_temporal=False))
    got = gpu_ctx.track_batch(streams, kw)
    for i, (pair, ext) in enumerate(cases):
        for k in FIELDS:
            assert _same(got[i][k], alone[i][k]), (pair, ext, k)
    for s in streams:
        s.close()
