"""k_track4 at its arithmetic and geometric edges, bit for bit against the CPU oracle: the case sets of
tests/lk_cases.py (saturated images, displacements that force re-staging, the per-level border gates, ten image sizes)
through mskf_fe_track with and without the temporal half and with non-identity Hpred, the independence of a point from
its three wavefront neighbours, and mskf_fe_track_batch with mixed streams.  tests/test_lk_cases.py shows on the oracle
alone that the inputs reach what they are meant to reach."""
import numpy as np
import pytest

from msckf_stereo_c_amd import capi
from msckf_stereo_c_amd.ctypes_types import default_ekf_cfg, default_fe_cfg

import lk_cases as C

pytestmark = pytest.mark.gpu

SIZE_IDS = ["%dx%d" % s for s in C.SIZES]
FIELDS = ("out0", "out1", "und0", "und1", "status")


_bits, _same, _check = C.bits, C.same, C.check_track        # shared with tests/test_gpu_frame_counts.py


def _load(s, c):
    """prev cam0 = A, curr cam0 = B, curr cam1 = B1."""
    s.push_stereo(c["A"], c["A"])
    s.swap()
    s.push_stereo(c["B"], c["B1"])


@pytest.mark.parametrize("set_name", sorted(C.CASE_SETS))
@pytest.mark.parametrize("w,h", C.SIZES, ids=SIZE_IDS)
def test_lk_case_set_bit_exact(gpu_ctx, oracle, set_name, w, h):
    """Every case of the set at this size, with the temporal half (Hpred of the case) and without it."""
    calib, fe = oracle.euroc_calib(w, h), default_fe_cfg()
    n_ok = n_in = 0
    for c in C.cases(set_name, w, h, oracle):
        s = capi.Stream(gpu_ctx, calib, fe, default_ekf_cfg())        # a stream of its own per image pair; reuse has its own test
        _load(s, c)
        a, b = _check(s.track(c["pts"], do_temporal=True, Hpred=c["H"]), oracle, calib, fe, c, True, (c["name"], "temporal"))
        n_ok += a
        n_in += b
        _check(s.track(c["pts"], do_temporal=False), oracle, calib, fe, c, False, (c["name"], "stereo only"))
        s.close()
    print("%dx%d %s: %d tracked, %d stereo inliers" % (w, h, set_name, n_ok, n_in))
    # the stereo half must not degenerate either: the cam1 image is the cam0 image moved along the epipolar lines, so a good
    # share of the tracked points passes the epipolar gate (tests/test_lk_cases.py holds the floor for n_ok)
    assert n_ok > 0 and n_in >= max(1, n_ok // 4)


@pytest.mark.parametrize("models", [(1, 1), (0, 1)])
def test_lk_equidistant_model_at_an_odd_size(gpu_ctx, oracle, models):
    """The equidistant model in the stereo guess, the gates and the undistorted outputs at 333 x 251, both cameras and
    the (radtan, equidistant) pair."""
    w, h = 333, 251
    calib, fe = oracle.euroc_calib(w, h), default_fe_cfg()
    calib.cam0_model, calib.cam1_model = models
    fish = (-0.013, 0.021, -0.008, 0.0015)          # Kannala-Brandt k1..k4 of a mild fisheye
    for i in range(4):
        if models[0] == 1: calib.cam0_distortion[i] = fish[i]
        if models[1] == 1: calib.cam1_distortion[i] = fish[i] * 0.9
    n_in = 0
    for c in C.cases("sizes", w, h, oracle) + C.cases("border", w, h, oracle)[:1]:
        s = capi.Stream(gpu_ctx, calib, fe, default_ekf_cfg())
        _load(s, c)
        n_in += _check(s.track(c["pts"], do_temporal=True, Hpred=c["H"]), oracle, calib, fe, c, True, c["name"])[1]
        _check(s.track(c["pts"], do_temporal=False), oracle, calib, fe, c, False, c["name"])
        s.close()
    assert n_in > 10


@pytest.mark.parametrize("set_name,name", [("displaced", "regions1"), ("displaced", "shift_mx"), ("saturated", "inverse"),
                                           ("saturated", "stripes4v8_shift1_0"), ("border", "border_guess_right")])
def test_lk_point_does_not_depend_on_its_wave_neighbours(gpu_ctx, oracle, set_name, name):
    """The four points of a wavefront share the iteration loop, the barriers and (when any of them asks) the re-staging:
    the same image pair with the points permuted and with n % 4 = 0, 1, 2, 3 gives every point the same bits."""
    w, h = 376, 240
    calib, fe = oracle.euroc_calib(w, h), default_fe_cfg()
    s = capi.Stream(gpu_ctx, calib, fe, default_ekf_cfg())
    c = [x for x in C.cases(set_name, w, h, oracle) if x["name"] == name][0]
    _load(s, c)
    pts = c["pts"]
    base = {t: s.track(pts, do_temporal=t, Hpred=c["H"]) for t in (True, False)}
    _check(base[True], oracle, calib, fe, c, True, c["name"])
    rng = np.random.default_rng(5)
    for drop in range(4):
        n = len(pts) // 4 * 4 - drop
        perm = rng.permutation(len(pts))[:n]
        for t in (True, False):
            got = s.track(pts[perm], do_temporal=t, Hpred=c["H"])
            for k in FIELDS:
                assert _same(got[k], base[t][k][perm]), (c["name"], drop, t, k)
    # and alone in its wavefront
    for i in range(0, len(pts), max(1, len(pts) // 16)):
        got = s.track(pts[i:i + 1], do_temporal=True, Hpred=c["H"])
        for k in FIELDS:
            assert _same(got[k], base[True][k][i:i + 1]), (c["name"], i, k)
    s.close()


def _batch_problems(oracle, n_streams):
    """Streams of three sizes with different point counts, mixed do_temporal and a different Hpred per temporal stream."""
    sizes = [(129, 71), (376, 240), (65, 67)]
    counts = [0, 1, 3, 4, 5, 63, 64, 257, 2, 1500, 7]
    src = {}
    for (w, h) in sizes:
        cs = C.cases("displaced", w, h, oracle)
        src[(w, h)] = [cs[-1], cs[6], cs[1]]        # regions, an Hpred case, a plain shift
    out = []
    for i in range(n_streams):
        w, h = sizes[i % 3]
        c = dict(src[(w, h)][(i // 3) % 3])
        reps = -(-counts[i] // max(1, len(c["pts"])))
        c["pts"] = np.ascontiguousarray(np.tile(c["pts"], (max(reps, 1), 1))[:counts[i]] + np.float32(0.125 * (i % 3)))
        do_temporal = i % 4 != 2
        if do_temporal and np.array_equal(c["H"], np.eye(3)):
            c["H"] = C.translation(0.5 * i, -0.25 * i)
        out.append((w, h, c, do_temporal))
    return out


@pytest.mark.parametrize("n_streams", [11, 8, 9])
def test_lk_track_batch_equals_single_calls_and_oracle(gpu_ctx, oracle, n_streams):
    """One mskf_fe_track_batch over streams of different sizes, point counts (0, 1, 3, 4, 5, 63, 64, 257, ...), temporal
    and stereo-only, each with its own Hpred: the block -> (stream, point group) mapping with a stream count that is
    and is not a multiple of 8.  Each stream's result equals the same call issued alone, and the oracle."""
    fe = default_fe_cfg()
    probs = _batch_problems(oracle, n_streams)
    streams = []
    for (w, h, c, _) in probs:
        s = capi.Stream(gpu_ctx, oracle.euroc_calib(w, h), fe, default_ekf_cfg())
        _load(s, c)
        streams.append(s)
    kw = [dict(pts=c["pts"], do_temporal=t, Hpred=c["H"]) for (_, _, c, t) in probs]
    got = gpu_ctx.track_batch(streams, kw)
    halves = gpu_ctx.track_batch_begin(streams, kw)          # the same in two halves
    gpu_ctx.track_batch_end()
    for i in range(len(streams)):
        for k in FIELDS:
            assert _same(halves[i][k], got[i][k]), (i, k)
    n_ok = 0
    for i, (s, (w, h, c, t)) in enumerate(zip(streams, probs)):
        alone = s.track(**kw[i])
        for k in FIELDS:
            assert len(got[i][k]) == len(c["pts"])
            assert _same(got[i][k], alone[k]), (i, k)
        n_ok += _check(got[i], oracle, s.calib, fe, c, t, ("stream", i))[0]
    assert n_ok > 100
    # an all-empty batch: OK, nothing pending, _end is a no-op
    empty = [dict(pts=np.zeros((0, 2), np.float32), do_temporal=True) for _ in streams]
    res = gpu_ctx.track_batch_begin(streams, empty)
    assert all(len(r["status"]) == 0 for r in res)
    gpu_ctx.track_batch_end()
    gpu_ctx.track_batch_end()
    assert len(streams[1].track(kw[1]["pts"], kw[1]["do_temporal"], kw[1]["Hpred"])["status"]) == len(kw[1]["pts"])
    for s in streams:
        s.close()


def test_lk_second_image_pair_on_a_reused_stream(gpu_ctx, oracle):
    """A stream loaded with one image pair after another (push, swap, push, each call straight after the other) holds
    the pyramids of exactly those images, all levels of all three roles, and tracks them as a stream of its own does: a
    push must not disturb the one before it, whose work may still be queued when it returns."""
    w, h = 333, 251
    calib, fe = oracle.euroc_calib(w, h), default_fe_cfg()
    s = capi.Stream(gpu_ctx, calib, fe, default_ekf_cfg())
    for c in C.cases("border", w, h, oracle)[:3]:
        _load(s, c)
        for role, img in ((0, c["A"]), (1, c["B"]), (2, c["B1"])):
            ref = oracle.build_pyramid(img)
            for lvl in range(4):
                assert np.array_equal(s.get_level(role, lvl), ref[lvl]), (c["name"], role, lvl)
        _check(s.track(c["pts"], do_temporal=True, Hpred=c["H"]), oracle, calib, fe, c, True, c["name"])
        _check(s.track(c["pts"], do_temporal=False), oracle, calib, fe, c, False, c["name"])
    s.close()
