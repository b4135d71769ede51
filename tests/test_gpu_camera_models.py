"""The opt-in camera models on the device (mskf_fe_set_camera_model; k_track4_ext) against the float64 restatement of the contract
bit for bit and the long-double model within the bars of tests/test_gpu_camera_geometry.py, on the cases tests/camera_models_cases.py
states and tests/test_camera_models_reference.py ran on the CPU: the flat-pair probe, mixed batches, the setter's protocol, the
runners on the synthetic sequences and the app's camchain forms.

  * Flat-pair probe (the trick of test_gpu_camera_geometry.py): on a constant 64 x 64 pair a stereo-only track call returns the
    stereo guess in out1, status 1, out0 = the input, und0 / und1 the undistortions.  A point whose guess cannot be formed takes no
    stereo trip (out1 = 0), a coordinate that cannot be computed is 0.
  * A mixed batch runs base-model streams through the extended instantiation: their bytes must be those of an all-base batch.

Observed on MI355X (24 tests, three seconds together): all 8 lens pairs and all 8 point counts equal the restatement bit for bit
(out0, out1, und0, und1, status); against the long-double model the worst well-conditioned coordinate is 0 ulp away and 0 of
1260 .. 1532 coordinates per stage and set differ from its rounding (cap 0.1 %), at most 2 of 766 points are ill conditioned (cap
2 % = 15), 118 .. 135 points of the fov / ds sets are outside the domain and come back as 0; the mixed batch of three base and seven
extended streams gives every stream its single-call bytes and the base streams their all-base bytes; the Runners on radtan8 with
k3 = 0 equal an untouched twin, those on a small k3 and on the fitted fov / ds lenses publish the restatement's coordinates on
every frame, run every frame after the first on the device, and pipelined == lockstep == stepped, device books == host books.
"""
import ctypes as C
import os

import numpy as np
import pytest

import camera_cases as CC
import camera_models_cases as MC
import camera_models_reference as M
import camera_reference as R
import mask_reference as MR
import test_gpu_fb as GF
import test_gpu_patch as GP
from msckf_stereo_c_amd import capi
from msckf_stereo_c_amd.ctypes_types import CAMERA_MODELS, FeCameraModel, default_ekf_cfg, default_fe_cfg

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not R.HAVE_LONG_DOUBLE, reason=R.NEED_LONG_DOUBLE)]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("out0", "out1", "und0", "und1", "status")
FLAT = np.full((64, 64), 128, np.uint8)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32) if a.dtype == np.float32 else a


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _status(f, *a, **kw):
    try:
        f(*a, **kw)
        return 0
    except capi.MskfError as e:
        return e.code


def _stream(gpu_ctx, case):
    s = capi.Stream(gpu_ctx, MC.calib(case), default_fe_cfg(), default_ekf_cfg())
    MC.apply_models(s, case)
    s.push_stereo(FLAT, FLAT)
    return s


def _flat_track(gpu_ctx, case, pts):
    s = _stream(gpu_ctx, case)
    got = s.track(pts, do_temporal=False)
    s.close()
    return got


def _equals_restatement(got, case, pts):
    exp = MC.expected(case, pts)
    for k in FIELDS:
        assert _same(got[k], exp[k]), (case, k, np.flatnonzero((_bits(got[k]) != _bits(exp[k])).reshape(len(pts), -1).any(1))[:8])
    return exp


# ------------------------------------------------------------------------------------------ flat-pair probe
@pytest.mark.parametrize("case", MC.CASE_NAMES)
def test_flat_pair_probe(gpu_ctx, case):
    pts = MC.point_set(case)
    got = _flat_track(gpu_ctx, case, pts)
    exp = _equals_restatement(got, case, pts)
    fig, bad = MC.judge(case, pts, got["out1"], got["und0"], got["und1"])
    print(MC.figures_line(case, fig))
    assert not bad, bad
    if case in ("fov", "ds", "ds_verged", "fov_ds"):
        out = ~exp["guessed"]
        assert out.sum() > 20 and (got["out1"][out] == 0).all() and (got["status"] == 1).all()


@pytest.mark.parametrize("n", MC.COUNTS)
def test_point_counts(gpu_ctx, n):
    """Four points share a wavefront and the geometry is computed once per 16-lane row: counts around both, on a pair of two
    extended models with points outside the domain among the first ones."""
    pts = MC.point_set("fov_ds")
    order = np.argsort(-np.abs(pts - 256.0).max(1), kind="stable")          # rim and outside-the-domain points first
    sel = np.ascontiguousarray(pts[order][:n]).reshape(-1, 2)
    s = _stream(gpu_ctx, "fov_ds")
    if n == 0:
        assert gpu_ctx.track_batch([s], [dict(pts=sel, do_temporal=False)])[0]["status"].size == 0
    else:
        got = s.track(sel, do_temporal=False)
        exp = _equals_restatement(got, "fov_ds", sel)
        assert n < 4 or not exp["guessed"].all()
    s.close()


# ------------------------------------------------------------------------------------------ mixed batch
def test_mixed_batch(gpu_ctx):
    """radtan, equidistant and each new model in one mskf_fe_track_batch: every stream's bytes equal its single call; the
    base-model streams' bytes equal what the same streams give in an all-base batch (the extended instantiation's old arms)."""
    base = [("euroc", "euroc"), ("tumvi", "roll90"), ("kalibr", "vertical")]
    ext = ["cv5", "rational", "fov", "ds_verged", "fov_ds", "cv5_radtan", "equi_rational"]
    streams, kw = [], []
    for pair, e in base:
        s = capi.Stream(gpu_ctx, CC.calib(pair, e, 64, 64), default_fe_cfg(), default_ekf_cfg())
        s.push_stereo(FLAT, FLAT)
        streams.append(s)
        kw.append(dict(pts=np.ascontiguousarray(CC.point_set(pair, e)[0]), do_temporal=False))
    all_base = gpu_ctx.track_batch(streams, kw)
    for case in ext:
        streams.append(_stream(gpu_ctx, case))
        kw.append(dict(pts=np.ascontiguousarray(MC.point_set(case)), do_temporal=False))
    alone = [s.track(k["pts"], do_temporal=False) for s, k in zip(streams, kw)]
    order = [3, 0, 4, 1, 5, 6, 2, 7, 8, 9]                                  # base and extended streams interleaved
    got = gpu_ctx.track_batch([streams[i] for i in order], [kw[i] for i in order])
    for j, i in enumerate(order):
        for k in FIELDS:
            assert _same(got[j][k], alone[i][k]), (i, k)
            if i < len(base):
                assert _same(got[j][k], all_base[i][k]), (i, k)
    for i, case in enumerate(ext):
        _equals_restatement(alone[len(base) + i], case, kw[len(base) + i]["pts"])
    for s in streams:
        s.close()


# ------------------------------------------------------------------------------------------ setter protocol
def test_set_camera_model_protocol(gpu_ctx, oracle):
    L = gpu_ctx.L
    L.mskf_fe_set_camera_model.argtypes = [C.c_void_p, C.c_void_p]
    L.mskf_fe_get_camera_model.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    L.mskf_abi_version.restype = C.c_int
    assert L.mskf_abi_version() == 4
    c = CC.calib("radtan_equi", "verged", 64, 64)
    pts = np.ascontiguousarray(CC.point_set("radtan_equi", "verged")[0])
    s = capi.Stream(gpu_ctx, c, default_fe_cfg(), default_ekf_cfg())
    s.push_stereo(FLAT, FLAT)
    never = s.track(pts, do_temporal=False)
    # a stream never set reports what mskf_calib gave it
    assert s.get_camera_model(0) == ("radtan", list(c.cam0_distortion) + [0.0] * 4)
    assert s.get_camera_model(1) == ("equidistant", list(c.cam1_distortion) + [0.0] * 4)
    s.set_camera_model(1, "ds", (-0.19, 0.61))
    held = ("ds", [-0.19, 0.61] + [0.0] * 6)
    assert s.get_camera_model(1) == held and s.get_camera_model(0)[0] == "radtan"
    with_ds = s.track(pts, do_temporal=False)
    assert not _same(with_ds["out1"], never["out1"]) and _same(with_ds["und0"], never["und0"])
    nan, inf, pi = float("nan"), float("inf"), float(np.pi)

    def cfg(cam, model, *k):
        return FeCameraModel(cam, model, (C.c_double * 8)(*(list(k) + [0.0] * (8 - len(k)))))
    bad = [cfg(2, 4, -0.2, 0.6), cfg(-1, 4, -0.2, 0.6), cfg(1, 5, 0.1), cfg(1, -1, 0.1), cfg(1, 2, nan), cfg(1, 2, 0, 0, 0, 0, 0, 0, 0, inf), cfg(1, 0, 0, nan),
           cfg(1, 3, 0.0), cfg(1, 3, -0.5), cfg(1, 3, pi), cfg(1, 3, 4.0), cfg(1, 3, nan), cfg(1, 4, -1.0, 0.5), cfg(1, 4, 1.0000001, 0.5), cfg(1, 4, 0.0, -0.001),
           cfg(1, 4, 0.0, 1.001), cfg(1, 4, 0.0, 0.5, inf)]
    for b in bad:
        assert L.mskf_fe_set_camera_model(s.h, C.byref(b)) == -1 and len(L.mskf_last_error()) > 0
        assert s.get_camera_model(1) == held and s.get_camera_model(0)[0] == "radtan"
    assert L.mskf_fe_set_camera_model(s.h, None) == -1 and L.mskf_fe_set_camera_model(None, None) == -1
    assert L.mskf_fe_get_camera_model(s.h, 1, None) == -1 and L.mskf_fe_get_camera_model(s.h, 2, C.byref(cfg(0, 0))) == -1
    for f in (lambda: s.set_camera_model(1, "omni", (1.0,)), lambda: s.set_camera_model(1, "fov", (0.9, 0.1)), lambda: s.set_camera_model(1, "radtan8", (0.1,) * 6)):
        assert _status(f) == -1 and s.get_camera_model(1) == held
    assert _same(s.track(pts, do_temporal=False)["out1"], with_ds["out1"])          # every refusal left the setting in force
    for good in [(0, "fov", (3.14159,)), (0, "ds", (1.0, 1.0)), (0, "ds", (-0.999, 0.0)), (0, "radtan8", (0.1, 0.2, 0.3, 0.4, 0.5)), (0, "radtan", list(c.cam0_distortion))]:
        s.set_camera_model(*good)
        assert s.get_camera_model(0) == (good[1], [float(v) for v in good[2]] + [0.0] * (8 - len(good[2])))
    # pending track batch: refused, the message names it
    gpu_ctx.track_batch_begin([s], [dict(pts=pts[:8], do_temporal=0)])
    try:
        assert _status(s.set_camera_model, 1, "fov", (0.9,)) == -1 and b"track batch" in L.mskf_last_error()
    finally:
        gpu_ctx.track_batch_end()
    assert s.get_camera_model(1) == held
    # back to the calibration's model and coefficients: never having set it, bitwise
    s.set_camera_model(1, "equidistant", list(c.cam1_distortion))
    again = s.track(pts, do_temporal=False)
    for k in FIELDS:
        assert _same(again[k], never[k]), k
    s.close()
    # pending device frame
    w, h = 188, 120
    syn = oracle.Synth(seed=0x5EED00D0, width=w, height=h)
    a, b = syn.render(0)
    s = capi.Stream(gpu_ctx, syn.calib, default_fe_cfg(), default_ekf_cfg())
    s.push_stereo(a, b)
    cm = s.cell_maxima()
    p = np.stack([cm["x"], cm["y"]], 1)[cm["score"] > 2560][:60].astype(np.float32)
    s.track(p, 0)
    s.swap()
    s.set_grid()
    gpu_ctx.frame_batch_begin([s], [(a, b)], [{}])
    try:
        assert _status(s.set_camera_model, 0, "fov", (0.9,)) == -1 and b"device frame" in L.mskf_last_error()
    finally:
        gpu_ctx.frame_batch_end()
    assert s.get_camera_model(0)[0] == "radtan"
    s.set_camera_model(0, "fov", (0.9,))
    assert s.get_camera_model(0) == ("fov", [0.9] + [0.0] * 7)
    s.close()


# ------------------------------------------------------------------------------------------ runners
class _Rig:
    """A synthetic sequence under another calibration (the images stay the rig's own)."""

    def __init__(self, syn, calib):
        self._syn, self.calib = syn, calib

    def __getattr__(self, name):
        return getattr(self._syn, name)


def _lens(oracle, kind):
    """(calib, [(cam, model, coeffs), ...]) of a Runner test on the rig at the small test size."""
    from msckf_stereo_c_amd.ctypes_types import Calib
    w, h = GP._RUN["w"], GP._RUN["h"]
    base = oracle.euroc_calib(w, h)
    calib = Calib.from_buffer_copy(bytes(base))
    K = [list(base.cam0_intrinsics), list(base.cam1_intrinsics)]
    D = [list(base.cam0_distortion), list(base.cam1_distortion)]
    if kind == "radtan8_zero":
        return calib, [(c, "radtan8", D[c] + [0.0] * 4) for c in (0, 1)]
    if kind == "k3":
        return calib, [(0, "radtan8", D[0] + [-0.004]), (1, "radtan8", D[1] + [-0.0035, 0.0, 0.0, 0.0])]
    model = dict(fov=M.FOV, ds=M.DS)[kind]
    sets = []
    for c in (0, 1):
        p, Kf, _ = MC.fit_to_radtan(K[c], D[c], (w, h), model)
        for i in range(4):
            (calib.cam0_intrinsics if c == 0 else calib.cam1_intrinsics)[i] = Kf[i]
        sets.append((c, kind, p))
    return calib, sets


def _set(r, sets, stream=None):
    for c, model, k in sets:
        r.set_camera_model(c, model, k, stream=stream)


def _published_match_restatement(run, calib, sets):
    """Every feature of the last message: its normalised coordinates are the restatement's undistortion of its pixels."""
    ids, _, c0, c1 = run.dump(0)[:4]
    msg = run.msg(0)[:len(ids)]          # (the message's first records are this frame's; stale and zero records follow: quirk Q1)
    assert len(msg) == len(ids) >= 1 and sorted(int(i) for i in msg["id"]) == sorted(int(i) for i in ids)
    at = {int(i): k for k, i in enumerate(ids)}
    idx = np.array([at[int(i)] for i in msg["id"]])
    cams = {c: (CAMERA_MODELS[m], k) for c, m, k in sets}
    for c, px, u, v in ((0, c0, "u0", "v0"), (1, c1, "u1", "v1")):
        K = list(calib.cam0_intrinsics if c == 0 else calib.cam1_intrinsics)
        model, k = cams[c]
        p = np.stack([px["x"], px["y"]], 1).astype(np.float32)[idx]
        want, ok = M.undistort64(K, model, k, p)
        assert ok.all()
        assert _same(np.stack([msg[u], msg[v]], 1).astype(np.float32), want), c
        assert np.array_equal(np.stack([msg[u], msg[v]], 1), want.astype(np.float64))
    return len(msg)


@GF._guarded
def test_runner_radtan8_with_zero_k3_equals_an_untouched_twin(oracle):
    syn = oracle.Synth(seed=GP._RUN["seed"], width=GP._RUN["w"], height=GP._RUN["h"])
    _, sets = _lens(oracle, "radtan8_zero")
    keep = []
    plain = GP._sequence_run(oracle, [syn], keep)
    twin = GP._sequence_run(oracle, [syn], keep, setup=lambda r: _set(r, sets))
    assert len(plain.dump(0)[0]) > 10
    GP._same_run(twin, plain)
    assert np.array_equal(twin.msg(0), plain.msg(0)) and len(twin.msg(0)) >= len(twin.dump(0)[0])
    for r in (plain, twin):
        r.close()


@GF._guarded
@pytest.mark.parametrize("kind", ["k3", "fov", "ds"])
def test_runner_on_an_extended_model(oracle, kind):
    """Every published feature's normalised coordinates equal the restatement's undistortion of its pixels, every frame after the
    first is a device frame, device books == host books; pipelined == lockstep == the frame-by-frame run; a second stream of the
    batch that keeps the calibration's model is untouched."""
    w, h, n_frames = GP._RUN["w"], GP._RUN["h"], GP._RUN["n_frames"]
    calib, sets = _lens(oracle, kind)
    syn = _Rig(oracle.Synth(seed=GP._RUN["seed"], width=w, height=h), calib)
    other = _Rig(oracle.Synth(seed=GP._RUN["seed"] + 1, width=w, height=h), calib)
    frames = [syn.render(k) for k in range(n_frames)]
    state = dict(n=0, runs=None)

    def setup(r):
        _set(r, sets)
        state["runs"] = (state["runs"] or []) + [r]

    def on_frame(k, d):
        assert len(d[0]) >= 1, k
        state["n"] += _published_match_restatement(state["runs"][0], calib, sets)
    runs = GP._stepped_runs(syn, frames, setup, on_frame)          # (asserts device frames, and device books == host books)
    assert state["n"] > 5 * n_frames
    keep = []
    plain = GP._sequence_run(oracle, [syn, other], keep)
    for pipelined in (False, True):
        run = GP._sequence_run(oracle, [syn, other], keep, pipelined=pipelined, setup=lambda r: _set(r, sets, stream=0))
        GP._same_run(run, runs[0])
        GP._same_run(run, plain, 1, 1)                      # the stream that keeps the calibration's model is untouched
        run.close()
    n = len(runs[0].dump(0)[0])
    assert not np.array_equal(plain.msg(0)[:n], runs[0].msg(0)[:n])
    plain.close()
    for r in runs:
        r.close()


@GF._guarded
def test_runner_with_mask_patch_and_fb_checks_on_an_extended_model(oracle):
    """The three gates behind the extended launch as behind the base one: with a mask, the patch check and the forward-backward
    check on together with a radtan8 lens, the published features pass each gate's restatement and the camera model's."""
    w, h, n_frames = GP._RUN["w"], GP._RUN["h"], GP._RUN["n_frames"]
    calib, sets = _lens(oracle, "k3")
    syn = _Rig(oracle.Synth(seed=GP._RUN["seed"], width=w, height=h), calib)
    frames = [syn.render(k) for k in range(n_frames)]
    mask = np.ones((h, w), np.uint8)
    mask[:, :12] = 0
    usable = MR.erode(MR.usable_of(mask), 2)
    state = dict(before=None, n=0, runs=None)

    def setup(r):
        _set(r, sets)
        r.set_mask(cam0=mask, margin=2)
        r.set_patch_check("both", GP._RUN["half"], GP._RUN["tt"], GP._RUN["ts"])
        r.set_fb_check("both", GF._FB["tt"], GF._FB["ts"])
        state["runs"] = (state["runs"] or []) + [r]

    def on_frame(k, d):
        assert len(d[0]) >= 1, k
        state["n"] += _published_match_restatement(state["runs"][0], calib, sets)
        GP._published_pass(frames, k, d, state["before"], GP._RUN["half"], GP._RUN["tt"], GP._RUN["ts"])
        GF._published_pass(frames, k, d, state["before"])
        c0 = d[2]
        assert usable[MR.pixel(c0["y"]), MR.pixel(c0["x"])].all(), k
        state["before"] = d
    runs = GP._stepped_runs(syn, frames, setup, on_frame)
    assert state["n"] > 2 * n_frames
    for r in runs:
        r.close()


# ------------------------------------------------------------------------------------------ the app
@GF._guarded
def test_app_reads_the_camchain_forms(tmp_path, oracle):
    """A camchain with five distortion coefficients and one with camera_model: ds through the headless app on a few frames: the
    tracking counts it logs are those of a Runner set the same way, frame for frame."""
    import shutil
    import subprocess
    from PIL import Image
    from msckf_stereo_c_amd import build
    from msckf_stereo_c_amd import runner as RN
    from msckf_stereo_c_amd.ctypes_types import Calib, EkfCfg, FeCfg, ImuSample
    build.build_all()
    n_frames, w, h = 6, 752, 480
    syn = oracle.Synth(seed=0x5EED0042, width=w, height=h, n_static=3, motion_scale=3.0)
    mav0 = tmp_path / "mav0"
    for c in (0, 1):
        (mav0 / ("cam%d" % c) / "data").mkdir(parents=True)
    (mav0 / "imu0").mkdir()
    t0_ns, dt_ns = 1403715273262142976, 50000000
    rows, frames = [], []
    for k in range(n_frames):
        a, b = syn.render(k)
        frames.append((a, b))
        name = "%d.png" % (t0_ns + k * dt_ns)
        Image.fromarray(a).save(mav0 / "cam0" / "data" / name, compress_level=1)
        Image.fromarray(b).save(mav0 / "cam1" / "data" / name, compress_level=1)
        rows.append("%d,%s\r" % (t0_ns + k * dt_ns, name))
    for c in (0, 1):
        (mav0 / ("cam%d" % c) / "data.csv").write_text("#timestamp [ns],filename\r\n" + "\n".join(rows) + "\n")
    lines = ["#timestamp [ns],w_x,w_y,w_z,a_x,a_y,a_z"]
    for j in range((n_frames + 2) * 10):
        s = syn.imu(j)
        vals = list(s.angular_velocity) + list(s.linear_acceleration)
        lines.append("%d,%s" % (t0_ns + j * (dt_ns // 10), ",".join("%.9g" % v for v in vals)))
    (mav0 / "imu0" / "data.csv").write_text("\n".join(lines) + "\n")
    exe = os.path.join(ROOT, "msckf_stereo_c_amd", "_build", "run_euroc_single_thread")
    chain = (open(os.path.join(ROOT, "config", "camchain-imucam-euroc.yaml")).read())
    base = syn.calib
    D0, D1 = list(base.cam0_distortion), list(base.cam1_distortion)
    K1 = list(base.cam1_intrinsics)
    fmt = lambda v: "[" + ", ".join(repr(float(x)) for x in v) + "]"

    def stamp(ns):
        return (int(str(ns)[:-9]) * 1e9 + int(str(ns)[-9:])) * 1e-9
    imu = []
    for line in lines[1:]:
        f = line.split(",")
        v = [float(np.float32(x)) for x in f[1:7]]
        imu.append(ImuSample(stamp(int(f[0])), (C.c_double * 3)(*v[:3]), (C.c_double * 3)(*v[3:])))

    def rewrite(text, cam, repl):
        """Replace (or, with None, drop) one-line keys of one camera's block of the camchain text."""
        out, inside = [], False
        for line in text.splitlines():
            if line and not line[0].isspace():
                inside = line.startswith(cam + ":")
            key = line.strip().split(":")[0]
            if inside and line[:1].isspace() and key in repl:
                if repl[key] is not None:
                    out.append("  %s: %s" % (key, repl[key]))
                continue
            out.append(line)
        return "\n".join(out) + "\n"

    ds1 = (-0.21, 0.59)
    variants = {
        "five": (rewrite(chain, "cam0", {"distortion_coeffs": fmt(D0 + [-0.004])}), [(0, "radtan8", D0 + [-0.004])]),
        "ds": (rewrite(chain, "cam1", {"camera_model": "ds", "distortion_model": None, "distortion_coeffs": None,
                                        "intrinsics": fmt(list(ds1) + [0.62 * K1[0], 0.62 * K1[1], K1[2], K1[3]])}), [(1, "ds", list(ds1))]),
    }
    for tag, (text, sets) in variants.items():
        cfg = tmp_path / tag / "config"
        shutil.copytree(os.path.join(ROOT, "config"), cfg)
        (cfg / "camchain-imucam-euroc.yaml").write_text(text)
        work = tmp_path / tag / "build"
        work.mkdir()
        res = subprocess.run([exe, str(mav0)], cwd=work, capture_output=True, text=True, timeout=120)
        assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
        log = (work / "debug_imageprocessor.txt").read_text().strip().splitlines()
        got = [tuple(int(v) for v in line.split(":")[1].split(",")) for line in log]
        calib, fe, ekf = Calib(), FeCfg(), EkfCfg()
        assert RN.lib().mskfh_load_configs(str(cfg).encode(), C.byref(calib), C.byref(fe), C.byref(ekf)) == 0
        want = {}
        for on in (True, False):
            run = RN.Runner(calib, fe, ekf, 1, 1)
            if on:
                _set(run, sets)
            view = RN.StreamView(run)
            j, out = 0, []
            for k in range(n_frames):
                t_img = stamp(t0_ns + k * dt_ns)
                while True:
                    smp = imu[j]
                    j += 1
                    view.imu(smp)
                    if not (smp.time_stamp <= t_img):
                        break
                view.stereo(frames[k][0], frames[k][1], t_img)
                view.backend()
                info = run.dump(0)[4]
                out.append((info.before_tracking, info.after_tracking, info.after_matching, info.after_ransac))
            if on:
                _published_match_restatement(run, calib, sets + [(c, "radtan", list(calib.cam0_distortion if c == 0 else calib.cam1_distortion))
                                                                 for c in (0, 1) if c not in [s_[0] for s_ in sets]])
            run.close()
            want[on] = out
        assert len(got) > 2 and got == want[True][-len(got):], (tag, got, want[True])
        if tag == "ds":
            assert want[True] != want[False]
