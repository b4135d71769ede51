"""Every opt-in setting of a track pass at once (image mask, ZNCC patch check, forward-backward check, an extended camera model,
deeper LK pyramids; DESIGN.md section 3, "A frame of a group"): the only case in which the staged segments of a track batch (seven)
and of a device frame (eight) no longer fit one staging-copy launch.  A track batch against the gates' restatements applied, in
the pass's order, to the outputs of the same batch without mask and checks; the one-call device frame against the phased path;
the setters in two orders.  Only the public Python API is used."""
import numpy as np
import pytest

import deep_lk_reference as D
import fb_reference as FB
import mask_reference as MR
import patch_reference as PR
import test_gpu_fb as GF
import test_gpu_patch as GP
import test_patch_reference as TP
from msckf_stereo_c_amd import capi
from msckf_stereo_c_amd.ctypes_types import default_ekf_cfg, default_fe_cfg

pytestmark = pytest.mark.gpu

K_LK, K_GATES = 2, 12                         # MSKF_K_LK; the slot MSKF_K_FE_MASK, MSKF_K_FE_PATCH and MSKF_K_FE_FB share
NAMES = GP.NAMES
SHAPES = [(188, 120), (376, 240), (188, 120)] # a plain stream, the stream with every option, a stream with the patch check only
ALL, PATCH_ONLY, PLAIN = 1, 2, 0
HALF, LEVELS = 3, 5                           # five levels: the most 376 x 240 allows (level 4 is 24 x 15)
_CACHE = {}


def _radtan8(calib):
    """The radtan8 lens of test_gpu_camera_models' combined test: the calibration's radtan plus a k3, in both coefficient counts."""
    return [(0, "radtan8", list(calib.cam0_distortion) + [-0.004]), (1, "radtan8", list(calib.cam1_distortion) + [-0.0035, 0.0, 0.0, 0.0])]


def _pairs(oracle):
    if "pairs" not in _CACHE:
        syn = {sh: oracle.Synth(seed=0x5EED00B0 + sh[0], width=sh[0], height=sh[1]) for sh in set(SHAPES)}
        _CACHE["pairs"] = [syn[sh].render(k) for k, sh in enumerate(SHAPES)]
    return _CACHE["pairs"]


def _run(gpu_ctx, oracle, name, setup):
    """(pts, results, launches) of one stereo-only track_batch over fresh streams of SHAPES that `setup` has configured; computed once
    per name."""
    if name not in _CACHE:
        pairs = _pairs(oracle)
        ss = [capi.Stream(gpu_ctx, oracle.euroc_calib(w, h), default_fe_cfg(), default_ekf_cfg()) for (w, h) in SHAPES]
        try:
            setup(ss)
            gpu_ctx.push_stereo_batch(ss, [p[0] for p in pairs], [p[1] for p in pairs])
            gpu_ctx.sync()
            cms = [s.cell_maxima() for s in ss]
            pts = [np.stack([cm["x"][cm["score"] > 2560], cm["y"][cm["score"] > 2560]], 1)[:70 + 35 * k].astype(np.float32) for k, cm in enumerate(cms)]
            with GP._Timed(gpu_ctx) as t:
                res = gpu_ctx.track_batch(ss, [dict(pts=p, do_temporal=0) for p in pts])
        finally:
            for s in ss:
                s.close()
        _CACHE[name] = (pts, res, t.launches)
    return _CACHE[name]


def _lens_and_levels(ss):
    for c, model, k in _radtan8(ss[ALL].calib):
        ss[ALL].set_camera_model(c, model, k)
    ss[ALL].set_lk_levels(LEVELS)


def _unchecked(gpu_ctx, oracle):
    """The batch with the camera model and the levels set, no mask and no checks, and what the second batch is configured from:
    the cam1 mask under every fifth stereo inlier of the all-on stream, the patch thresholds of both checking streams (medians over
    what reaches the patch gate) and the forward-backward threshold (the median round trip, at the stream's depth, of what reaches
    that gate)."""
    if "derived" not in _CACHE:
        pairs = _pairs(oracle)
        pts, res, launches = _run(gpu_ctx, oracle, "unchecked", _lens_and_levels)
        w, h = SHAPES[ALL]
        r = res[ALL]
        ok = np.flatnonzero(r["status"] == 3)
        u1 = np.ones((h, w), bool)
        u1[MR.pixel(r["out1"][ok[::5], 1]), MR.pixel(r["out1"][ok[::5], 0])] = False
        masked = MR.gate(None, MR.pack(u1), w, h, *[r[n] for n in NAMES])
        thr_p = {}
        for k, st in ((ALL, masked[4]), (PATCH_ONLY, res[PATCH_ONLY]["status"])):
            ok = np.flatnonzero(st == 3)
            thr_p[k] = TP.median_threshold(GP._zncc(pairs[k][0], res[k]["out0"][ok], pairs[k][1], res[k]["out1"][ok], HALF))
            assert thr_p[k] is not None, k
        patched = PR.gate(None, pairs[ALL][0], pairs[ALL][1], 3, HALF, 1.0, thr_p[ALL], 0, pts[ALL], *masked)
        ok = np.flatnonzero(patched[4] == 3)
        back, st = D.lk_track(pairs[ALL][1], pairs[ALL][0], patched[1][ok], patched[0][ok], LEVELS)
        d = (back - patched[0][ok]).astype(np.float64)
        err = np.sort(np.hypot(d[:, 0], d[:, 1])[st != 0])
        assert len(err) >= 20
        thr_fb = float(np.float32(err[len(err) // 2]))
        assert 0.0 < thr_fb <= FB.MAX_ERROR
        _CACHE["derived"] = dict(u1=u1, thr_p=thr_p, thr_fb=thr_fb)
    return _CACHE["unchecked"], _CACHE["derived"]


def _all_on(gpu_ctx, oracle, name, reverse):
    """The batch with everything on; `reverse`: the all-on stream's setters are called in the opposite order."""
    _, d = _unchecked(gpu_ctx, oracle)

    def setup(ss):
        s = ss[ALL]
        setters = [lambda: s.set_lk_levels(LEVELS)]
        setters += [lambda c=c, m=m, k=k: s.set_camera_model(c, m, k) for c, m, k in _radtan8(s.calib)]
        setters += [lambda: s.set_mask(cam1=d["u1"]),
                    lambda: s.set_patch_check("both", HALF, 1.0, d["thr_p"][ALL]),        # (a stereo-only call: the temporal halves do not run)
                    lambda: s.set_fb_check("both", 0.0, d["thr_fb"])]
        for f in (reversed(setters) if reverse else setters):
            f()
        ss[PATCH_ONLY].set_patch_check("stereo", HALF, 0.0, d["thr_p"][PATCH_ONLY])
    return _run(gpu_ctx, oracle, name, setup)


@GF._guarded
def test_track_batch_with_every_option(gpu_ctx, oracle, monkeypatch):
    """One stream of a track batch carries a cam1 mask, both patch checks, both forward-backward checks, a radtan8 lens and five LK
    levels (seven staged segments: two staging-copy launches); a plain stream and a patch-checking one sit beside it.  The all-on
    stream's five output arrays are, byte for byte, mask_reference.gate, then patch_reference.gate, then fb_reference.gate (its LK the
    restatement at five levels) applied to the outputs of the same batch with only the lens and the levels set.  Each gate refuses
    some points and at least ten keep status 3; the plain stream is untouched; one track launch, three gate launches."""
    pairs = _pairs(oracle)
    pts_n, res_n, t_n = _run(gpu_ctx, oracle, "nothing", lambda ss: None)
    (pts0, res0, t0), d = _unchecked(gpu_ctx, oracle)
    pts1, res1, t1 = _all_on(gpu_ctx, oracle, "all_on", False)
    assert t_n[K_LK] == 1 and t_n[K_GATES] == 0
    assert t0[K_LK] == 1 and t0[K_GATES] == 0
    assert t1[K_LK] == 1 and t1[K_GATES] == 3                        # mask gate, patch gate, forward-backward gate
    for k in range(len(SHAPES)):
        assert np.array_equal(pts_n[k], pts0[k]) and np.array_equal(pts0[k], pts1[k]), k
    assert len(pts1[ALL]) > 80
    w, h = SHAPES[ALL]
    before = [res0[ALL][n] for n in NAMES]
    masked = MR.gate(None, MR.pack(d["u1"]), w, h, *before)
    patched = PR.gate(None, pairs[ALL][0], pairs[ALL][1], 3, HALF, 1.0, d["thr_p"][ALL], 0, pts1[ALL], *masked)
    monkeypatch.setattr(FB, "_lk", lambda a, b, p, g: D.lk_track(a, b, p, g, LEVELS))
    want = FB.gate(None, pairs[ALL][0], pairs[ALL][1], 3, 0.0, d["thr_fb"], 0, pts1[ALL], *patched)
    changed = [int((a[4] != b[4]).sum()) for a, b in ((masked, before), (patched, masked), (want, patched))]
    print("all-on stream: %d points, %d with status 3 unchecked; the gates change %s, %d keep status 3" %
          (len(pts1[ALL]), int((before[4] == 3).sum()), changed, int((want[4] == 3).sum())))
    assert min(changed) >= 1 and (want[4] == 3).sum() >= 10
    for name, a in zip(NAMES, want):
        assert a.tobytes() == res1[ALL][name].tobytes(), name
    # the patch-checking stream: its own gate on its unchecked outputs; the plain stream: as in a batch with nothing set
    before = [res0[PATCH_ONLY][n] for n in NAMES]
    want = PR.gate(None, pairs[PATCH_ONLY][0], pairs[PATCH_ONLY][1], 2, HALF, 0.0, d["thr_p"][PATCH_ONLY], 0, pts1[PATCH_ONLY], *before)
    assert (want[4] != before[4]).sum() >= 10 and (want[4] == 3).sum() >= 10
    for name, a in zip(NAMES, want):
        assert a.tobytes() == res1[PATCH_ONLY][name].tobytes(), name
    for name in NAMES:
        assert res_n[PLAIN][name].tobytes() == res0[PLAIN][name].tobytes() == res1[PLAIN][name].tobytes(), name
        assert res_n[PATCH_ONLY][name].tobytes() == res0[PATCH_ONLY][name].tobytes(), name
    # the lens and the depth are on in the unchecked batch: its all-on stream is not the default stream's
    assert any(res_n[ALL][name].tobytes() != res0[ALL][name].tobytes() for name in NAMES)


@GF._guarded
def test_setter_order_does_not_matter(gpu_ctx, oracle):
    """The all-on stream configured levels, lens, mask, patch check, forward-backward check, and in the opposite order: the batch
    gives identical bytes for every stream."""
    pts1, res1, t1 = _all_on(gpu_ctx, oracle, "all_on", False)
    pts2, res2, t2 = _all_on(gpu_ctx, oracle, "all_on_reversed", True)
    assert t2[K_LK] == 1 and t2[K_GATES] == 3
    for k in range(len(SHAPES)):
        assert np.array_equal(pts1[k], pts2[k])
        for name in NAMES:
            assert res1[k][name].tobytes() == res2[k][name].tobytes(), (k, name)


@GF._guarded
def test_runner_device_frames_equal_the_phased_path_with_every_option(oracle):
    """A Runner with the five options on over the synthetic sequence of test_gpu_lk_levels: every frame after the first is a one-call
    device frame (eight staged segments), and it publishes, bit for bit, what the same sequence gives through the phased path of the
    host mirror (books on the host, mskf_fe_track_batch)."""
    from msckf_stereo_c_amd import runner as R
    w, h, n_frames = 752, 480, 6
    syn = oracle.Synth(seed=0x5EED0042, width=w, height=h, n_static=3, motion_scale=3.0)
    frames = [syn.render(k) for k in range(n_frames)]
    mask = np.ones((h, w), np.uint8)
    mask[:, :12] = 0
    runs = []
    try:
        for host in (0, 1):                           # device books (the one-call device frame), host books (the phased path)
            R.set_fe_books_on_host(host)
            r = R.Runner(syn.calib, default_fe_cfg(), default_ekf_cfg(max_cam_state_size=10), 1, 1)
            runs.append(r)
            r.set_lk_levels(6)
            for c, model, k in _radtan8(syn.calib):
                r.set_camera_model(c, model, k)
            r.set_mask(cam0=mask, cam1=mask, margin=2)
            r.set_patch_check("both", GP._RUN["half"], GP._RUN["tt"], GP._RUN["ts"])
            r.set_fb_check("both", GF._FB["tt"], GF._FB["ts"])
        j = n_tracked = 0
        for k in range(n_frames):
            t_img = syn.frame_time(k)
            while True:
                smp = syn.imu(j)
                j += 1
                for r in runs:
                    r.imu(0, smp)
                if not (smp.time_stamp <= t_img):
                    break
            for host, r in zip((0, 1), runs):
                R.set_fe_books_on_host(host)
                r.step([frames[k][0]], [frames[k][1]], [t_img])
            d0, d1 = runs[0].dump(0), runs[1].dump(0)
            i0, i1 = d0[4], d1[4]
            print("frame %d: %d features, tracking %d -> %d -> %d -> %d" % (k, len(d0[0]), i0.before_tracking, i0.after_tracking, i0.after_matching, i0.after_ransac))
            for x, y in zip(d0[:4], d1[:4]):
                assert x.tobytes() == y.tobytes(), k
            assert (i0.before_tracking, i0.after_tracking, i0.after_matching, i0.after_ransac) == (i1.before_tracking, i1.after_tracking, i1.after_matching, i1.after_ransac)
            assert len(d0[0]) > 10, k
            n_tracked += i0.after_matching
        assert runs[0].num_device_frames() == n_frames - 1 and runs[1].num_device_frames() == 0
        assert n_tracked > 0                          # (the checks are tight: what matters is that points reach every gate on both paths)
    finally:
        R.set_fe_books_on_host(-1)
        for r in runs:
            r.close()
