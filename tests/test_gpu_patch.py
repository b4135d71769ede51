"""Opt-in ZNCC patch check on the device (mskf_fe_set_patch_check; k_patch_points) against the numpy restatement of the contract
(tests/patch_reference.py; DESIGN.md §3, "Patch check"), bit for bit: the gate launched directly between guard bytes and behind
real track calls, mixed batches, the setter's protocol, the runners and the app's YAML keys."""
import ctypes as C
import os

import numpy as np
import pytest

import mask_reference as MR
import patch_reference as PR
import test_patch_reference as TP
from msckf_stereo_c_amd import capi
from msckf_stereo_c_amd.ctypes_types import FePatchCheck, default_ekf_cfg, default_fe_cfg
from test_gpu_detector_edges import FeStreamDev

from hip_runtime import Hip

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K_LK, K_FE_PATCH, K_COUNT = 2, 12, 14         # MSKF_K_LK, MSKF_K_FE_PATCH (the slot of MSKF_K_PT_GEOM, shared with the mask gate), MSKF_K_COUNT
_HIP_ERRORS = []                              # after a HIP error no test of this module launches anything
NAMES = ("out0", "out1", "und0", "und1", "status")


class FePatchDev(C.Structure):
    """FePatchDev of csrc/hip/fe_patch.h: element i goes with descriptor i of a launch."""
    _fields_ = [("thr2_t", C.c_double), ("thr2_s", C.c_double), ("half", C.c_int), ("mode", C.c_int)]


def test_fe_patch_dev_layout_matches_the_header(tmp_path):
    import subprocess
    so = str(tmp_path / "libfe_patch_test.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-I", ROOT, "-o", so, os.path.join(ROOT, "tests", "cpp", "fe_patch_test.cpp")])
    out = (C.c_int * 8)()
    n = C.CDLL(so).fp_patch_dev_layout(out, 8)
    assert list(out[:n]) == [C.sizeof(FePatchDev)] + [getattr(FePatchDev, k).offset for k in ("thr2_t", "thr2_s", "half", "mode")]


def _ok_to_launch():
    assert not _HIP_ERRORS, "an earlier launch ended with a HIP error: %s" % _HIP_ERRORS


def _guarded(test):
    """A test that launches: it does not start after a HIP error of an earlier one, and records its own (an error of the library
    other than a refused argument, or anything that is neither that nor a failed assertion)."""
    import functools

    @functools.wraps(test)
    def run(*a, **kw):
        _ok_to_launch()
        try:
            return test(*a, **kw)
        except AssertionError:
            raise
        except capi.MskfError as e:
            if e.code not in (-1, -4):
                _HIP_ERRORS.append(repr(e))
            raise
        except BaseException as e:
            _HIP_ERRORS.append(repr(e))
            raise
    return run


# ------------------------------------------------------------------------------------------ the gate, launched directly
DIRECT_SIZES = [(40, 33), (17, 17)]
IMG_SEED = 11


def _direct_specs():
    """(n, size index, half, mode, do_temporal, device-side count or None) per descriptor."""
    specs = [(n, 0, 4, 3, 1, None) for n in (0, 1, 3, 4, 5, 63, 64, 65, 257)] + [(257, 0, 4, 3, 1, 100)]
    k = 0
    for half in (2, 4, 7):
        for mode in (1, 2, 3):
            for do_temporal in (1, 0):
                specs.append((65, k % 2, half, mode, do_temporal, None))
                k += 1
                if len(specs) == 20:
                    specs.append((65, 1, 4, 0, 1, None))                  # mode 0 between two checking descriptors
    return specs


def _gate_direct(gpu_ctx, max_pts):
    """One fe_launch_patch_points over the descriptors of _direct_specs.  Every array (the images and the input points too) lies
    between guard bytes in one buffer, which is compared whole with the restatement's."""
    _ok_to_launch()
    specs = _direct_specs()
    images = [TP.gate_images(w, h, IMG_SEED) for (w, h) in DIRECT_SIZES]
    hip = Hip()
    f = gpu_ctx.L.fe_launch_patch_points
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    f.restype = None
    try:
        total = 64
        img_off = []
        for (w, h) in DIRECT_SIZES:
            o = []
            for _ in range(3):
                o.append(total)
                total += (w * h + 63) // 64 * 64 + 64
            img_off.append(o)
        offs = []
        for n, *_ in specs:
            o = {}
            for name, size in (("in_pts", 8 * n), ("out0", 8 * n), ("out1", 8 * n), ("und0", 8 * n), ("und1", 8 * n), ("status", n), ("count", 4)):
                o[name] = total
                total += (size + 63) // 64 * 64 + 64
            offs.append(o)
        host = np.full(total, 0xA5, np.uint8)
        for o, imgs in zip(img_off, images):
            for off, img in zip(o, imgs):
                host[off:off + img.size] = img.reshape(-1)
        want = host.copy()
        changed = survived = 0
        for k, ((n, si, half, mode, do_temporal, count), o) in enumerate(zip(specs, offs)):
            w, h = DIRECT_SIZES[si]
            arrs = list(TP.gate_points(w, h, n, 1000 + k, do_temporal))              # in_pts, out0, out1, und0, und1, status
            m = n if count is None else count
            gated = PR.gate(*images[si], mode, half, TP.GATE_T[0], TP.GATE_T[1], do_temporal, *[a[:m] for a in arrs])
            exp = [arrs[0]] + [np.concatenate([g, a[m:]]) for g, a in zip(gated, arrs[1:])]
            changed += int((exp[5] != arrs[5]).sum())
            survived += int((exp[5][:m] != 0).sum())
            if mode == 0:
                assert all(a.tobytes() == e.tobytes() for a, e in zip(arrs, exp))
            for name, a, e in zip(("in_pts",) + NAMES, arrs, exp):
                host[o[name]:o[name] + a.nbytes] = a.reshape(-1).view(np.uint8)
                want[o[name]:o[name] + e.nbytes] = e.reshape(-1).view(np.uint8)
            cnt = np.array([0 if count is None else count], np.int32).view(np.uint8)
            host[o["count"]:o["count"] + 4] = cnt
            want[o["count"]:o["count"] + 4] = cnt
        assert changed > 50 and survived > 50
        d_buf = hip.alloc(total, False)
        hip.put(d_buf, host)
        desc, patch = (FeStreamDev * len(specs))(), (FePatchDev * len(specs))()
        for d, p, (n, si, half, mode, do_temporal, count), o in zip(desc, patch, specs, offs):
            w, h = DIRECT_SIZES[si]
            for pyr, off in zip((d.prev0, d.curr0, d.curr1), img_off[si]):
                pyr.lvl[0], pyr.w[0], pyr.h[0] = d_buf + off, w, h
            d.n_pts = n
            d.n_pts_dev = None if count is None else d_buf + o["count"]
            d.do_temporal = do_temporal
            d.in_pts = d_buf + o["in_pts"]
            d.out0, d.out1, d.und0, d.und1, d.status = (d_buf + o[k] for k in NAMES)
            p.thr2_t, p.thr2_s, p.half, p.mode = PR.thr2(TP.GATE_T[0]), PR.thr2(TP.GATE_T[1]), half, mode
        raw_d, raw_p = np.frombuffer(bytes(desc), np.uint8).copy(), np.frombuffer(bytes(patch), np.uint8).copy()
        d_desc, d_patch = hip.alloc(raw_d.size, False), hip.alloc(raw_p.size, False)
        hip.put(d_desc, raw_d)
        hip.put(d_patch, raw_p)
        f(d_desc, d_patch, len(specs), max_pts, gpu_ctx.hip_stream())
        gpu_ctx.sync()
        err = hip.last_error()
        assert err == 0, "hipGetLastError %d after k_patch_points" % err
        got = hip.get(d_buf, total)
    except BaseException as e:
        _HIP_ERRORS.append(repr(e))
        raise
    finally:
        hip.free()
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "bytes %s differ from the restatement (guards, images and untouched fields included)" % bad[:16]


@pytest.mark.parametrize("max_pts", [257, 4])
@_guarded
def test_gate_direct(gpu_ctx, max_pts):
    """max_pts = 257: a row of lanes per point; 4: the launch is cut from an estimate below the counts, a block takes several
    point groups."""
    _gate_direct(gpu_ctx, max_pts)


# ------------------------------------------------------------------------------------------ timing kinds
def _timing(ctx):
    L = ctx.L
    L.mskf_ctx_set_timing.argtypes = [C.c_void_p, C.c_int]
    L.mskf_ctx_get_timing.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    ms, n_l, n_u = np.zeros(K_COUNT), np.zeros(K_COUNT, np.int64), np.zeros(K_COUNT, np.int64)
    assert L.mskf_ctx_get_timing(ctx.h, ms.ctypes.data, n_l.ctypes.data, n_u.ctypes.data, 1) == 0
    return n_l


class _Timed:
    """with _Timed(ctx) as t: ...; t.launches[kind] afterwards."""

    def __init__(self, ctx):
        self.ctx = ctx

    def __enter__(self):
        _ok_to_launch()
        self.ctx.L.mskf_ctx_set_timing.argtypes = [C.c_void_p, C.c_int]
        assert self.ctx.L.mskf_ctx_set_timing(self.ctx.h, 1) == 0
        _timing(self.ctx)
        return self

    def __exit__(self, *exc):
        if exc[0] is not None:
            return False
        self.launches = _timing(self.ctx)
        self.ctx.L.mskf_ctx_set_timing(self.ctx.h, 0)
        return False


def _stream(ctx, oracle, w, h):
    return capi.Stream(ctx, oracle.euroc_calib(w, h), default_fe_cfg(), default_ekf_cfg())


def _zncc(img_a, pa, img_b, pb, half):
    return PR.zncc(PR.sums(img_a, pa[:, 0], pa[:, 1], img_b, pb[:, 0], pb[:, 1], half), half)


# ------------------------------------------------------------------------------------------ the gate behind a real track
@pytest.mark.parametrize("do_temporal", [1, 0])
@_guarded
def test_gate_behind_a_real_track(gpu_ctx, oracle, do_temporal):
    w, h, half, frame = TP.REAL["w"], TP.REAL["h"], TP.REAL["half"], TP.REAL["frame"]
    syn = oracle.Synth(seed=TP.REAL["seed"], width=w, height=h)
    s = _stream(gpu_ctx, oracle, w, h)
    prev0 = syn.render(frame)[0]
    s.push_stereo(*syn.render(frame))
    pts = TP.real_track_points(s.cell_maxima())
    assert len(pts) > 40
    curr0, curr1 = syn.render(frame)
    if do_temporal:
        s.swap()
        curr0, curr1 = syn.render(frame + 1)
        s.push_stereo(curr0, curr1)
    assert s.get_patch_check() == (0, 4, float(np.float32(0.8)), float(np.float32(0.8)))
    with _Timed(gpu_ctx) as t0:
        r0 = s.track(pts, do_temporal)
    assert t0.launches[K_FE_PATCH] == 0 and t0.launches[K_LK] == 1
    alive, matched = np.flatnonzero(r0["status"] & 1), np.flatnonzero(r0["status"] & 2)
    # thresholds from the restatement on the ungated outputs: at least ten points fail and ten pass each comparison
    tt = TP.median_threshold(_zncc(prev0, pts[alive], curr0, r0["out0"][alive], half)) if do_temporal else 0.5
    assert tt is not None
    mid = PR.gate(prev0, curr0, curr1, 1, half, tt, 0.0, do_temporal, pts, *[r0[n] for n in NAMES])
    still = np.flatnonzero(mid[4] & 2)
    ts = TP.median_threshold(_zncc(curr0, r0["out0"][still], curr1, r0["out1"][still], half))
    assert ts is not None
    want = PR.gate(prev0, curr0, curr1, 3, half, tt, ts, do_temporal, pts, *[r0[n] for n in NAMES])
    lost, unmatched = (r0["status"] != 0) & (want[4] == 0), ((r0["status"] & 2) != 0) & (want[4] == 1)
    assert (lost.sum() >= 10 and (mid[4] & 1).sum() >= 10) or not do_temporal
    assert unmatched.sum() >= 10 and (want[4] == 3).sum() >= 10
    s.set_patch_check("both", half, tt, ts)
    with _Timed(gpu_ctx) as t1:
        r1 = s.track(pts, do_temporal)
    assert t1.launches[K_FE_PATCH] == 1 and t1.launches[K_LK] == 1
    for name, a in zip(NAMES, want):
        assert a.tobytes() == r1[name].tobytes(), name
    # one comparison at a time
    for mode, m in (("temporal", 1), ("stereo", 2)):
        s.set_patch_check(mode, half, tt, ts)
        r = s.track(pts, do_temporal)
        for name, a in zip(NAMES, PR.gate(prev0, curr0, curr1, m, half, tt, ts, do_temporal, pts, *[r0[n] for n in NAMES])):
            assert a.tobytes() == r[name].tobytes(), (mode, name)
    s.set_patch_check("off")
    with _Timed(gpu_ctx) as t2:
        r2 = s.track(pts, do_temporal)
    assert t2.launches[K_FE_PATCH] == 0
    assert all(r0[n].tobytes() == r2[n].tobytes() for n in r0)
    s.close()


# ------------------------------------------------------------------------------------------ mixed batch
@_guarded
def test_mixed_batch(gpu_ctx, oracle):
    """track_batch over five streams of two sizes: two check (stereo / both), one is masked and checks, two are plain.  The plain
    streams equal a batch with nothing set, bit for bit; the checking ones the restatement on that batch's outputs; the masked
    and checking one the mask gate, then the patch gate.  The gates' timing slot counts 0, then 2 launches (mask gate, patch gate)."""
    shapes = [(188, 120), (376, 240), (188, 120), (376, 240), (188, 120)]
    half = 3
    syn = {sh: oracle.Synth(seed=0x5EED00B0 + sh[0], width=sh[0], height=sh[1]) for sh in set(shapes)}
    pairs = [syn[sh].render(k) for k, sh in enumerate(shapes)]

    def run(setup):
        ss = [_stream(gpu_ctx, oracle, w, h) for (w, h) in shapes]
        setup(ss)
        gpu_ctx.push_stereo_batch(ss, [p[0] for p in pairs], [p[1] for p in pairs])
        gpu_ctx.sync()
        cms = [s.cell_maxima() for s in ss]
        pts = [np.stack([cm["x"][cm["score"] > 2560], cm["y"][cm["score"] > 2560]], 1)[:70 + 17 * k].astype(np.float32) for k, cm in enumerate(cms)]
        with _Timed(gpu_ctx) as t:
            res = gpu_ctx.track_batch(ss, [dict(pts=p, do_temporal=0) for p in pts])
        for s in ss:
            s.close()
        return pts, res, t.launches

    pts0, res0, t0 = run(lambda ss: None)
    assert t0[K_FE_PATCH] == 0 and t0[K_LK] == 1
    assert len({len(p) for p in pts0}) == 5 and all((r["status"] == 3).sum() > 20 for r in res0)
    thr, u1 = [], None
    for k in range(3):
        ok = np.flatnonzero(res0[k]["status"] == 3)
        if k == 2:           # the masked stream: cam1 masked out under every fifth match; the threshold from what the mask gate leaves
            w, h = shapes[k]
            u1 = np.ones((h, w), bool)
            u1[MR.pixel(res0[k]["out1"][ok[::5], 1]), MR.pixel(res0[k]["out1"][ok[::5], 0])] = False
            ok = np.flatnonzero(MR.gate(None, MR.pack(u1), w, h, *[res0[k][n] for n in NAMES])[4] == 3)
        t = TP.median_threshold(_zncc(pairs[k][0], res0[k]["out0"][ok], pairs[k][1], res0[k]["out1"][ok], half))
        assert t is not None
        thr.append(t)

    def setup(ss):
        ss[0].set_patch_check("stereo", half, 0.0, thr[0])
        ss[1].set_patch_check("both", half, 1.0, thr[1])          # (a stereo-only call: the temporal comparison does not run)
        ss[2].set_mask(cam1=u1)
        ss[2].set_patch_check("both", half, 1.0, thr[2])
    pts1, res1, t1 = run(setup)
    assert t1[K_FE_PATCH] == 2 and t1[K_LK] == 1
    for k in range(5):
        assert np.array_equal(pts0[k], pts1[k])
        before = [res0[k][n] for n in NAMES]
        if k == 2:
            before = MR.gate(None, MR.pack(u1), shapes[k][0], shapes[k][1], *before)
            assert (before[4] != res0[k]["status"]).sum() >= 4
        if k < 3:
            want = PR.gate(None, pairs[k][0], pairs[k][1], 3 if k else 2, half, 1.0, thr[k], 0, pts0[k], *before)
            assert (want[4] != before[4]).sum() >= 10 and (want[4] == 3).sum() >= 10
        else:
            want = before
        for name, a in zip(NAMES, want):
            assert a.tobytes() == res1[k][name].tobytes(), (k, name)


# ------------------------------------------------------------------------------------------ protocol
def _status(call, *a, **kw):
    try:
        call(*a, **kw)
        return 0
    except capi.MskfError as e:
        return e.code


@_guarded
def test_set_patch_check_protocol(gpu_ctx, oracle):
    """Every refusal leaves the previous setting in force (get_patch_check); the setter is refused while a track batch or a device
    frame of the context is pending (the message names it) and accepted after its _end; mode 0 = off."""
    w, h = 188, 120
    L = gpu_ctx.L
    L.mskf_fe_set_patch_check.argtypes = [C.c_void_p, C.c_void_p]
    L.mskf_fe_get_patch_check.argtypes = [C.c_void_p, C.c_void_p]
    syn = oracle.Synth(seed=0x5EED00D0, width=w, height=h)
    a, b = syn.render(0)
    s = _stream(gpu_ctx, oracle, w, h)
    f08 = float(np.float32(0.8))
    assert s.get_patch_check() == (0, 4, f08, f08)
    s.set_patch_check("temporal", 5, 0.75, 0.25)
    held = (1, 5, 0.75, 0.25)
    assert s.get_patch_check() == held
    nan, inf = float("nan"), float("inf")
    for bad in [FePatchCheck(4, 4, 0.5, 0.5), FePatchCheck(7, 4, 0.5, 0.5), FePatchCheck(-1, 4, 0.5, 0.5), FePatchCheck(3, 1, 0.5, 0.5), FePatchCheck(1, 8, 0.5, 0.5),
                FePatchCheck(2, 0, 0.5, 0.5), FePatchCheck(2, -4, 0.5, 0.5), FePatchCheck(3, 4, -0.001, 0.5), FePatchCheck(3, 4, 0.5, 1.001), FePatchCheck(3, 4, nan, 0.5),
                FePatchCheck(3, 4, 0.5, nan), FePatchCheck(3, 4, inf, 0.5), FePatchCheck(3, 4, 0.5, -inf), FePatchCheck(0, 4, 2.0, 0.5), FePatchCheck(0, 4, 0.5, nan)]:
        assert L.mskf_fe_set_patch_check(s.h, C.byref(bad)) == -1 and len(L.mskf_last_error()) > 0
        assert s.get_patch_check() == held
    assert L.mskf_fe_set_patch_check(s.h, None) == -1 and L.mskf_fe_set_patch_check(None, None) == -1 and L.mskf_fe_get_patch_check(s.h, None) == -1
    assert _status(s.set_patch_check, "sometimes") == -1 and s.get_patch_check() == held
    # the limits are accepted; with mode 0 any half is
    for good in [(3, 2, 0.0, 1.0), (3, 7, 1.0, 0.0), (0, 99, 0.5, 0.5), (0, 0, 0.0, 0.0)]:
        s.set_patch_check(*good)
        assert s.get_patch_check() == good
    s.set_patch_check(*held)
    # pending track batch
    s.push_stereo(a, b)
    gpu_ctx.track_batch_begin([s], [dict(pts=np.array([[40.0, 40.0], [90.0, 60.0]]), do_temporal=0)])
    try:
        assert _status(s.set_patch_check, "both") == -1 and b"track batch" in L.mskf_last_error()
        assert _status(s.set_patch_check, "off") == -1
    finally:
        gpu_ctx.track_batch_end()
    assert s.get_patch_check() == held
    s.set_patch_check("stereo", 3, 0.5, 0.5)
    s.set_patch_check(*held)
    # pending device frame: refused, then accepted after its _end
    s.swap()
    s.set_grid()
    gpu_ctx.frame_batch_begin([s], [(a, b)], [{}])
    try:
        assert _status(s.set_patch_check, "both") == -1 and b"device frame" in L.mskf_last_error()
    finally:
        gpu_ctx.frame_batch_end()
    assert s.get_patch_check() == held
    s.set_patch_check("both")
    assert s.get_patch_check() == (3, 4, f08, f08)
    s.set_patch_check("off")
    assert s.get_patch_check()[0] == 0
    s.close()


# ------------------------------------------------------------------------------------------ runners
_RUN = dict(w=188, h=120, n_frames=30, seed=0x5EED00E0, half=4, tt=0.97, ts=0.8)


def _check(r, stream=None):
    r.set_patch_check("both", _RUN["half"], _RUN["tt"], _RUN["ts"], stream=stream)


def _same_run(a, b, i=0, j=0):
    for x, y in zip(a.dump(i)[:4], b.dump(j)[:4]):
        assert np.array_equal(x, y)
    pa, pb = a.poses(i), b.poses(j)
    assert len(pa) == len(pb) > 5
    assert np.array_equal(pa["t"], pb["t"]) and np.array_equal(pa["p"], pb["p"]) and np.array_equal(pa["q"], pb["q"])
    assert np.array_equal(a.cov(i), b.cov(j))


def _sequence_run(oracle, syns, keep, pipelined=False, setup=None):
    from msckf_stereo_c_amd import runner as R
    from test_gpu_system import _attach_sequences
    _ok_to_launch()
    run = R.Runner(syns[0].calib, default_fe_cfg(), default_ekf_cfg(max_cam_state_size=10), 1, len(syns), host_threads=1)
    if setup:
        setup(run)
    _attach_sequences(oracle, run, syns, _RUN["n_frames"], keep)
    run.run(0, _RUN["n_frames"], threaded=True, pipelined=pipelined)
    return run


def _published_pass(frames, k, dump, before, half, tt, ts):
    """Every feature of frame k's dump passes the stereo comparison on frame k's images, and every one that frame k - 1 published
    too the temporal comparison against its pixel there."""
    ids, life, c0, c1 = dump[:4]
    a, b = frames[k]
    p0, p1 = np.stack([c0["x"], c0["y"]], 1), np.stack([c1["x"], c1["y"]], 1)
    assert PR.decide(PR.sums(a, p0[:, 0], p0[:, 1], b, p1[:, 0], p1[:, 1], half), half, PR.thr2(ts)).all(), k
    n_tracked = 0
    if before is not None:
        was = {int(i): (x, y) for i, x, y in zip(before[0], before[2]["x"], before[2]["y"])}
        sel = np.array([int(i) in was for i in ids], bool)
        assert np.array_equal(sel, life > 1)
        pin = np.array([was[int(i)] for i in ids[sel]], np.float32).reshape(-1, 2)
        assert PR.decide(PR.sums(frames[k - 1][0], pin[:, 0], pin[:, 1], a, p0[sel, 0], p0[sel, 1], half), half, PR.thr2(tt)).all(), k
        n_tracked = int(sel.sum())
    return n_tracked


def _stepped_runs(syn, frames, setup, on_frame=None):
    """A device-books and a host-books Runner of one stream stepped frame by frame; on_frame(k, dump of the first)."""
    from msckf_stereo_c_amd import runner as R
    _ok_to_launch()
    n_frames = len(frames)
    runs = []
    try:
        for host in (0, 1):
            R.set_fe_books_on_host(host)
            r = R.Runner(syn.calib, default_fe_cfg(), default_ekf_cfg(max_cam_state_size=10), 1, 1)
            setup(r)
            runs.append(r)
        j = 0
        for k in range(n_frames):
            t_img = syn.frame_time(k)
            while True:
                s = syn.imu(j)
                j += 1
                for r in runs:
                    r.imu(0, s)
                if not (s.time_stamp <= t_img):
                    break
            a, b = frames[k]
            for host, r in zip((0, 1), runs):
                R.set_fe_books_on_host(host)
                r.step([a], [b], [t_img])
            d0, d1 = runs[0].dump(0), runs[1].dump(0)
            for x, y in zip(d0[:4], d1[:4]):
                assert np.array_equal(x, y), k
            i0, i1 = d0[4], d1[4]
            assert (i0.before_tracking, i0.after_tracking, i0.after_matching, i0.after_ransac) == (i1.before_tracking, i1.after_tracking, i1.after_matching, i1.after_ransac)
            if on_frame:
                on_frame(k, d0)
        assert runs[0].num_device_frames() == n_frames - 1 and runs[1].num_device_frames() == 0
        pa, pb = runs[0].poses(0), runs[1].poses(0)
        assert len(pa) == len(pb) > 5 and np.array_equal(pa["p"], pb["p"]) and np.array_equal(pa["q"], pb["q"])
    finally:
        R.set_fe_books_on_host(-1)
    return runs


@_guarded
def test_runner_checked(oracle):
    """Every published feature of every frame passes the restatement on the stream's own images, every frame publishes features
    and every frame after the first is a device frame; pipelined == lockstep == the frame-by-frame run, device books == host
    books, bit for bit; the check removes something; a second stream without the check is untouched."""
    w, h, n_frames = _RUN["w"], _RUN["h"], _RUN["n_frames"]
    syn = oracle.Synth(seed=_RUN["seed"], width=w, height=h)
    other = oracle.Synth(seed=_RUN["seed"] + 1, width=w, height=h)
    frames = [syn.render(k) for k in range(n_frames)]
    state = dict(before=None, tracked=0)

    def on_frame(k, d):
        assert len(d[0]) >= 1, k
        state["tracked"] += _published_pass(frames, k, d, state["before"], _RUN["half"], _RUN["tt"], _RUN["ts"])
        state["before"] = d
    runs = _stepped_runs(syn, frames, _check, on_frame)
    assert state["tracked"] > 10 * n_frames
    keep = []
    plain = _sequence_run(oracle, [syn, other], keep)
    for pipelined in (False, True):
        run = _sequence_run(oracle, [syn, other], keep, pipelined=pipelined, setup=lambda r: _check(r, stream=0))
        _same_run(run, runs[0])
        _same_run(run, plain, 1, 1)                         # the stream that does not check is untouched
        run.close()
    # ... and the check matters: the unchecked run publishes something else
    ids_p, ids_c = plain.dump(0)[0], runs[0].dump(0)[0]
    assert not np.array_equal(ids_p, ids_c)
    info_p, info_c = plain.dump(0)[4], runs[0].dump(0)[4]
    assert (info_p.after_tracking, info_p.after_matching) != (info_c.after_tracking, info_c.after_matching)
    plain.close()
    for r in runs:
        r.close()


@_guarded
def test_runner_on_and_off_again_equals_never_on(oracle):
    syn = oracle.Synth(seed=_RUN["seed"], width=_RUN["w"], height=_RUN["h"])
    keep = []
    plain = _sequence_run(oracle, [syn], keep)

    def on_off(r):
        _check(r)
        r.set_patch_check("off")
    off = _sequence_run(oracle, [syn], keep, setup=on_off)
    assert len(plain.dump(0)[0]) > 10
    _same_run(off, plain)
    for r in (plain, off):
        r.close()


@_guarded
def test_runner_set_patch_check_refuses_bad_arguments(oracle):
    from msckf_stereo_c_amd import runner as R
    _ok_to_launch()
    syn = oracle.Synth(seed=1, width=188, height=120)
    run = R.Runner(syn.calib, default_fe_cfg(), default_ekf_cfg(), 1, 2)
    for bad in [dict(mode="sometimes"), dict(mode=4), dict(half=1), dict(half=8), dict(min_zncc_temporal=1.5), dict(min_zncc_stereo=-0.5),
                dict(min_zncc_stereo=float("nan")), dict(stream=2)]:
        with pytest.raises(capi.MskfError):
            run.set_patch_check(**bad)
    run.set_patch_check("stereo", stream=1)
    run.set_patch_check("off")
    run.close()


@_guarded
def test_runner_pasted_occluder(oracle):
    """A block of foreign texture pasted over cam1 only (chosen on the CPU: test_patch_reference): the unchecked runner publishes
    at least five features on it in every frame, the checking one (defaults: half 4, 0.8 / 0.8) none in any frame, device books
    and host books alike."""
    from msckf_stereo_c_amd import runner as R
    w, h, n_frames = TP.OCCLUDER["w"], TP.OCCLUDER["h"], TP.OCCLUDER["n_frames"]
    syn = oracle.Synth(seed=TP.OCCLUDER["seed"], width=w, height=h)
    frames = [(syn.render(k)[0], TP.occlude(syn.render(k)[1])) for k in range(n_frames)]
    counts = dict(plain=[], checked=[], outside=[])

    def on_checked(k, d):
        ins = TP.inside_occluder(d[3])
        counts["checked"].append(int(ins.sum()))
        counts["outside"].append(int((~ins).sum()))
        _published_pass(frames, k, d, None, 4, 0.8, 0.8)
    runs = _stepped_runs(syn, frames, lambda r: r.set_patch_check(), on_checked)
    for r in runs:
        r.close()
    _ok_to_launch()
    plain = R.Runner(syn.calib, default_fe_cfg(), default_ekf_cfg(max_cam_state_size=10), 1, 1)
    try:
        j = 0
        for k in range(n_frames):
            t_img = syn.frame_time(k)
            while True:
                s = syn.imu(j)
                j += 1
                plain.imu(0, s)
                if not (s.time_stamp <= t_img):
                    break
            plain.step([frames[k][0]], [frames[k][1]], [t_img])
            counts["plain"].append(int(TP.inside_occluder(plain.dump(0)[3]).sum()))
    finally:
        plain.close()
    assert min(counts["plain"]) >= 5, counts
    assert max(counts["checked"]) == 0, counts
    assert min(counts["outside"]) >= 5, counts


# ------------------------------------------------------------------------------------------ the app
@_guarded
def test_app_reads_patch_check_keys(tmp_path, oracle):
    """The headless app with the four patch_check keys in its app_imgproc.yaml logs the tracking counts of a Runner with the same
    setting, frame for frame, which are not those of a Runner without it (the app without the keys logs those)."""
    import shutil
    import subprocess
    from PIL import Image
    from msckf_stereo_c_amd import build
    from msckf_stereo_c_amd import runner as R
    from msckf_stereo_c_amd.ctypes_types import Calib, EkfCfg, FeCfg, ImuSample
    _ok_to_launch()
    build.build_all()
    n_frames, w, h = 10, 752, 480
    syn = oracle.Synth(seed=0x5EED0042, width=w, height=h, n_static=3, motion_scale=3.0)          # (moving from frame 3 on)
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
    half, tt, ts = 3, 0.95, 0.85

    def app(tag, keys):
        cfg = tmp_path / tag / "config"
        shutil.copytree(os.path.join(ROOT, "config"), cfg)
        with open(cfg / "app_imgproc.yaml", "a") as f:
            f.write("\n" + keys)
        work = tmp_path / tag / "build"
        work.mkdir()
        res = subprocess.run([exe, str(mav0)], cwd=work, capture_output=True, text=True, timeout=120)
        assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
        log = (work / "debug_imageprocessor.txt").read_text().strip().splitlines()
        return [tuple(int(v) for v in line.split(":")[1].split(",")) for line in log], work, cfg
    got_on, work, cfg = app("on", "patch_check: both\npatch_check_half: %d\npatch_check_min_zncc_temporal: %r\npatch_check_min_zncc_stereo: %r\n" % (half, tt, ts))
    got_off, _, _ = app("off", "")

    def stamp(ns):          # what the app parses: seconds * 1e9 + nanoseconds in double
        return (int(str(ns)[:-9]) * 1e9 + int(str(ns)[-9:])) * 1e-9
    imu = []
    for line in lines[1:]:
        f = line.split(",")
        v = [float(np.float32(x)) for x in f[1:7]]
        imu.append(ImuSample(stamp(int(f[0])), (C.c_double * 3)(*v[:3]), (C.c_double * 3)(*v[3:])))
    calib, fe, ekf = Calib(), FeCfg(), EkfCfg()
    assert R.lib().mskfh_load_configs(str(cfg).encode(), C.byref(calib), C.byref(fe), C.byref(ekf)) == 0

    def runner_counts(checked):
        run = R.Runner(calib, fe, ekf, 1, 1)
        if checked:
            run.set_patch_check("both", half, tt, ts)
        view = R.StreamView(run)
        j, out = 0, []
        for k in range(n_frames):
            t_img = stamp(t0_ns + k * dt_ns)
            while True:
                s = imu[j]
                j += 1
                view.imu(s)
                if not (s.time_stamp <= t_img):
                    break
            view.stereo(frames[k][0], frames[k][1], t_img)
            view.backend()
            info = run.dump(0)[4]
            out.append((info.before_tracking, info.after_tracking, info.after_matching, info.after_ransac))
        run.close()
        return out
    want_on, want_off = runner_counts(True), runner_counts(False)
    assert len(got_on) == len(got_off) > 5
    assert got_on == want_on[-len(got_on):] and got_off == want_off[-len(got_off):]
    assert got_on != got_off
    # fewer features survive the track with the check on than without
    assert sum(c[2] for c in want_on[1:]) < sum(c[2] for c in want_off[1:])
