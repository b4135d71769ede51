"""Opt-in forward-backward check on the device (mskf_fe_set_fb_check; k_fb_points) against the restatement of the contract
(tests/fb_reference.py, built on the oracle's LK; DESIGN.md §3, "Forward-backward check"), bit for bit: the gate launched
directly between guard bytes and behind real track calls, mixed batches, the setter's protocol, the runners and the app's YAML
keys.  The inputs are those tests/test_fb_reference.py chose on the CPU."""
import ctypes as C
import os

import numpy as np
import pytest

import fb_reference as FB
import mask_reference as MR
import patch_reference as PR
import test_fb_reference as TF
import test_gpu_patch as GP
from msckf_stereo_c_amd import capi
from msckf_stereo_c_amd.ctypes_types import FeFbCheck, default_ekf_cfg, default_fe_cfg
from test_fb_reference import FeFbDev
from test_gpu_detector_edges import FeStreamDev

from hip_runtime import Hip

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K_LK, K_FE_FB = 2, 12                         # MSKF_K_LK, MSKF_K_FE_FB (the slot of MSKF_K_PT_GEOM, shared with the other point gates)
_HIP_ERRORS = []                              # after a HIP error no test of this module launches anything
NAMES = ("out0", "out1", "und0", "und1", "status")


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
class _Buffer:
    """One host buffer of named, 64-byte aligned fields with 64 guard bytes (0xA5) between them."""

    def __init__(self):
        self.total, self.fields = 64, []

    def add(self, data):
        data = np.ascontiguousarray(data).reshape(-1).view(np.uint8)
        off = self.total
        self.fields.append((off, data))
        self.total += (data.size + 63) // 64 * 64 + 64
        return off

    def bytes(self):
        host = np.full(self.total, 0xA5, np.uint8)
        for off, data in self.fields:
            host[off:off + data.size] = data
        return host


def _direct_buffers(oracle):
    """(input buffer, expected buffer, descriptors as (spec, image offsets, field offsets)): images with all four pyramid levels,
    every array of every descriptor of TF.direct_specs, and the restatement's results in their place."""
    buf, want = _Buffer(), _Buffer()
    pyr_off = []
    for (w, h) in TF.DIRECT_SIZES:
        offs = []
        for img in TF.gate_images(w, h, TF.IMG_SEED):
            levels = oracle.build_pyramid(img)
            o = [(buf.add(lv), lv.shape[1], lv.shape[0]) for lv in levels]
            for lv in levels:
                want.add(lv)
            offs.append(o)
        pyr_off.append(offs)
    descs = []
    for k, spec in enumerate(TF.direct_specs()):
        n, si, mode, do_temporal, count, statuses = spec
        _, arrs, exp = TF.direct_case(k, spec)
        o = {}
        for name, a, e in zip(("in_pts",) + NAMES, arrs, exp):
            o[name] = buf.add(a)
            assert want.add(e) == o[name]
        cnt = np.array([0 if count is None else count], np.int32)
        o["count"] = buf.add(cnt)
        want.add(cnt)
        descs.append((spec, pyr_off[si], o))
    return buf.bytes(), want.bytes(), descs


def _gate_direct(gpu_ctx, oracle, max_pts):
    """One fe_launch_fb_points over the descriptors of TF.direct_specs.  Every array (the pyramids and the input points too) lies
    between guard bytes in one buffer, which is compared whole with the restatement's."""
    _ok_to_launch()
    host, want, descs = _direct_buffers(oracle)
    assert host.size == want.size
    hip = Hip()
    f = gpu_ctx.L.fe_launch_fb_points
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    f.restype = None
    try:
        d_buf = hip.alloc(host.size, False)
        hip.put(d_buf, host)
        desc, fb = (FeStreamDev * len(descs))(), (FeFbDev * len(descs))()
        for d, p, ((n, si, mode, do_temporal, count, statuses), pyrs, o) in zip(desc, fb, descs):
            for pyr, levels in zip((d.prev0, d.curr0, d.curr1), pyrs):
                for l, (off, w, h) in enumerate(levels):
                    pyr.lvl[l], pyr.w[l], pyr.h[l] = d_buf + off, w, h
            d.n_pts = n
            d.n_pts_dev = None if count is None else d_buf + o["count"]
            d.do_temporal = do_temporal
            d.in_pts = d_buf + o["in_pts"]
            d.out0, d.out1, d.und0, d.und1, d.status = (d_buf + o[k] for k in NAMES)
            p.thr2_t, p.thr2_s, p.mode = FB.thr2(TF.DIRECT_T[0]), FB.thr2(TF.DIRECT_T[1]), mode
        raw_d, raw_p = np.frombuffer(bytes(desc), np.uint8).copy(), np.frombuffer(bytes(fb), np.uint8).copy()
        d_desc, d_fb = hip.alloc(raw_d.size, False), hip.alloc(raw_p.size, False)
        hip.put(d_desc, raw_d)
        hip.put(d_fb, raw_p)
        f(d_desc, d_fb, len(descs), max_pts, gpu_ctx.hip_stream())
        gpu_ctx.sync()
        err = hip.last_error()
        assert err == 0, "hipGetLastError %d after k_fb_points" % err
        got = hip.get(d_buf, host.size)
    except BaseException as e:
        _HIP_ERRORS.append(repr(e))
        raise
    finally:
        hip.free()
    assert (got != host).sum() >= 50                      # the launch did something
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "bytes %s differ from the restatement (guards, pyramids and untouched fields included)" % bad[:16]


@pytest.mark.parametrize("max_pts", [257, 4])
@_guarded
def test_gate_direct(gpu_ctx, oracle, max_pts):
    """max_pts = 257: a block per point group; 4: the launch is cut from an estimate below the counts, a block walks several
    point groups."""
    _gate_direct(gpu_ctx, oracle, max_pts)


def _launch_points(gpu_ctx, oracle, si, arrs, mode=3):
    """fe_launch_fb_points over one descriptor of TF.DIRECT_SIZES[si] with the given arrays; returns the five output arrays."""
    _ok_to_launch()
    w, h = TF.DIRECT_SIZES[si]
    buf = _Buffer()
    pyrs = [[(buf.add(lv), lv.shape[1], lv.shape[0]) for lv in oracle.build_pyramid(img)] for img in TF.gate_images(w, h, TF.IMG_SEED)]
    o = {name: buf.add(a) for name, a in zip(("in_pts",) + NAMES, arrs)}
    host = buf.bytes()
    n = len(arrs[5])
    hip = Hip()
    f = gpu_ctx.L.fe_launch_fb_points
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    f.restype = None
    try:
        d_buf = hip.alloc(host.size, False)
        hip.put(d_buf, host)
        d, p = FeStreamDev(), FeFbDev(FB.thr2(TF.DIRECT_T[0]), FB.thr2(TF.DIRECT_T[1]), mode)
        for pyr, levels in zip((d.prev0, d.curr0, d.curr1), pyrs):
            for l, (off, lw, lh) in enumerate(levels):
                pyr.lvl[l], pyr.w[l], pyr.h[l] = d_buf + off, lw, lh
        d.n_pts, d.n_pts_dev, d.do_temporal, d.in_pts = n, None, 1, d_buf + o["in_pts"]
        d.out0, d.out1, d.und0, d.und1, d.status = (d_buf + o[k] for k in NAMES)
        raw_d, raw_p = np.frombuffer(bytes(d), np.uint8).copy(), np.frombuffer(bytes(p), np.uint8).copy()
        d_desc, d_fb = hip.alloc(raw_d.size, False), hip.alloc(raw_p.size, False)
        hip.put(d_desc, raw_d)
        hip.put(d_fb, raw_p)
        f(d_desc, d_fb, 1, n, gpu_ctx.hip_stream())
        gpu_ctx.sync()
        assert hip.last_error() == 0
        got = hip.get(d_buf, host.size)
    except BaseException as e:
        _HIP_ERRORS.append(repr(e))
        raise
    finally:
        hip.free()
    return [got[o[name]:o[name] + a.nbytes].view(a.dtype).reshape(a.shape).copy() for name, a in zip(NAMES, arrs[1:])]


@_guarded
def test_a_point_does_not_depend_on_its_wave_neighbours(gpu_ctx, oracle):
    """A failing and a passing point (both halves), alone and in every row position among three others: the same outputs."""
    si = 1
    w, h = TF.DIRECT_SIZES[si]
    arrs = TF.gate_points(w, h, 257, 77, 1, [3])
    exp = FB.gate(*TF.gate_images(w, h, TF.IMG_SEED), 3, TF.DIRECT_T[0], TF.DIRECT_T[1], 1, *arrs)
    failing, passing, half = np.flatnonzero(exp[4] == 0), np.flatnonzero(exp[4] == 3), np.flatnonzero(exp[4] == 1)
    assert len(failing) >= 3 and len(passing) >= 3 and len(half) >= 1
    for i in (failing[0], passing[0], half[0]):
        others = [j for j in (failing[1], passing[1], passing[2], failing[2]) if j != i][:3]
        alone = _launch_points(gpu_ctx, oracle, si, [a[[i]] for a in arrs])
        for name, a, e in zip(NAMES, alone, exp):
            assert a[0].tobytes() == e[i].tobytes(), (i, name)
        for pos in range(4):
            sel = others[:pos] + [i] + others[pos:]
            got = _launch_points(gpu_ctx, oracle, si, [a[sel] for a in arrs])
            for name, a, b in zip(NAMES, got, alone):
                assert a[pos].tobytes() == b[0].tobytes(), (i, pos, name)


# ------------------------------------------------------------------------------------------ the gate behind a real track
def _stream(ctx, oracle, w, h):
    return capi.Stream(ctx, oracle.euroc_calib(w, h), default_fe_cfg(), default_ekf_cfg())


@pytest.mark.parametrize("do_temporal", [1, 0])
@_guarded
def test_gate_behind_a_real_track(gpu_ctx, oracle, do_temporal):
    """Off: the gates' slot counts nothing.  Both / temporal / stereo: one launch, and the outputs are the restatement applied to
    the unchecked outputs.  Off again equals never on.  (Without the feature there is no setter: this test fails.)"""
    w, h = TF.OCCLUDER["w"], TF.OCCLUDER["h"]
    prev0, curr0, curr1 = TF.gpu_track_images(oracle, do_temporal)
    s = _stream(gpu_ctx, oracle, w, h)
    if do_temporal:
        s.push_stereo(prev0, prev0)
        pts = TF.gpu_track_points(s.cell_maxima())
        s.swap()
        s.push_stereo(curr0, curr1)
    else:
        s.push_stereo(curr0, curr1)
        pts = TF.gpu_track_points(s.cell_maxima())
    assert len(pts) > 100
    assert s.get_fb_check() == (0, 1.0, 1.0)
    with GP._Timed(gpu_ctx) as t0:
        r0 = s.track(pts, do_temporal)
    assert t0.launches[K_FE_FB] == 0 and t0.launches[K_LK] == 1
    before = [r0[n] for n in NAMES]
    want = FB.gate(prev0, curr0, curr1, 3, 1.0, 1.0, do_temporal, pts, *before)
    lost, unmatched = (r0["status"] != 0) & (want[4] == 0), (r0["status"] == 3) & (want[4] == 1)
    assert (lost.sum() >= 10) == bool(do_temporal) and unmatched.sum() >= 10 and (want[4] == 3).sum() >= 10
    s.set_fb_check("both")
    assert s.get_fb_check() == (3, 1.0, 1.0)
    with GP._Timed(gpu_ctx) as t1:
        r1 = s.track(pts, do_temporal)
    assert t1.launches[K_FE_FB] == 1 and t1.launches[K_LK] == 1
    for name, a in zip(NAMES, want):
        assert a.tobytes() == r1[name].tobytes(), name
    # one half at a time, at other thresholds
    for mode, m, tt, ts in (("temporal", 1, 0.5, 64.0), ("stereo", 2, 0.0, 0.25)):
        s.set_fb_check(mode, tt, ts)
        r = s.track(pts, do_temporal)
        one = FB.gate(prev0, curr0, curr1, m, tt, ts, do_temporal, pts, *before)
        assert (one[4] != r0["status"]).any() == bool(m == 2 or do_temporal)
        for name, a in zip(NAMES, one):
            assert a.tobytes() == r[name].tobytes(), (mode, name)
    s.set_fb_check("off")
    with GP._Timed(gpu_ctx) as t2:
        r2 = s.track(pts, do_temporal)
    assert t2.launches[K_FE_FB] == 0
    assert all(r0[n].tobytes() == r2[n].tobytes() for n in r0)
    s.close()


# ------------------------------------------------------------------------------------------ mixed batch
@_guarded
def test_mixed_batch(gpu_ctx, oracle):
    """track_batch over five streams of two sizes: one checks both, one stereo only, one is masked, patch-checked and forward-
    backward-checked, two are plain.  The plain streams equal a batch with nothing set, bit for bit; the others the mask ->
    patch -> forward-backward restatements in that order.  The gates' slot counts 0 with nothing set, then 3."""
    shapes = [(188, 120), (376, 240), (188, 120), (376, 240), (188, 120)]
    half, thr_s = 3, 0.03
    syn = {sh: oracle.Synth(seed=0x5EED00B0 + sh[0], width=sh[0], height=sh[1]) for sh in set(shapes)}
    pairs = [syn[sh].render(k) for k, sh in enumerate(shapes)]

    def run(setup):
        ss = [_stream(gpu_ctx, oracle, w, h) for (w, h) in shapes]
        setup(ss)
        gpu_ctx.push_stereo_batch(ss, [p[0] for p in pairs], [p[1] for p in pairs])
        gpu_ctx.sync()
        cms = [s.cell_maxima() for s in ss]
        pts = [np.stack([cm["x"][cm["score"] > 2560], cm["y"][cm["score"] > 2560]], 1)[:70 + 17 * k].astype(np.float32) for k, cm in enumerate(cms)]
        with GP._Timed(gpu_ctx) as t:
            res = gpu_ctx.track_batch(ss, [dict(pts=p, do_temporal=0) for p in pts])
        for s in ss:
            s.close()
        return pts, res, t.launches

    pts0, res0, t0 = run(lambda ss: None)
    assert t0[K_FE_FB] == 0 and t0[K_LK] == 1
    assert len({len(p) for p in pts0}) == 5 and all((r["status"] == 3).sum() > 20 for r in res0)
    # the masked stream: cam1 masked out under every fifth match; its patch threshold from what the mask gate leaves
    k = 2
    w, h = shapes[k]
    ok = np.flatnonzero(res0[k]["status"] == 3)
    u1 = np.ones((h, w), bool)
    u1[MR.pixel(res0[k]["out1"][ok[::5], 1]), MR.pixel(res0[k]["out1"][ok[::5], 0])] = False
    ok = np.flatnonzero(MR.gate(None, MR.pack(u1), w, h, *[res0[k][n] for n in NAMES])[4] == 3)
    z = np.sort(PR.zncc(PR.sums(pairs[k][0], res0[k]["out0"][ok, 0], res0[k]["out0"][ok, 1], pairs[k][1], res0[k]["out1"][ok, 0], res0[k]["out1"][ok, 1], half), half))
    thr_p = float(np.float32(np.clip(z[len(z) // 4], 0, 1)))          # the patch gate removes about a quarter of them

    def setup(ss):
        ss[0].set_fb_check("both", 1.0, thr_s)                        # (a stereo-only call: the temporal half does not run)
        ss[1].set_fb_check("stereo", 0.0, thr_s)
        ss[2].set_mask(cam1=u1)
        ss[2].set_patch_check("stereo", half, 1.0, thr_p)
        ss[2].set_fb_check("both", 0.0, thr_s)
    pts1, res1, t1 = run(setup)
    assert t1[K_FE_FB] == 3 and t1[K_LK] == 1                         # mask gate, patch gate, forward-backward gate
    for k in range(5):
        assert np.array_equal(pts0[k], pts1[k])
        before = [res0[k][n] for n in NAMES]
        if k == 2:
            masked = MR.gate(None, MR.pack(u1), shapes[k][0], shapes[k][1], *before)
            assert (masked[4] != before[4]).sum() >= 4
            before = PR.gate(None, pairs[k][0], pairs[k][1], 2, half, 1.0, thr_p, 0, pts0[k], *masked)
            assert (before[4] != masked[4]).sum() >= 4
        if k < 3:
            want = FB.gate(None, pairs[k][0], pairs[k][1], 3 if k != 1 else 2, 1.0, thr_s, 0, pts0[k], *before)
            assert (want[4] != before[4]).sum() >= 3 and (want[4] == 3).sum() >= 10, k
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
def test_set_fb_check_protocol(gpu_ctx, oracle):
    """Every refusal leaves the previous setting in force (get_fb_check); the setter is refused while a track batch or a device
    frame of the context is pending (the message names it) and accepted after its _end; a setting applies from the next call."""
    w, h = 188, 120
    L = gpu_ctx.L
    L.mskf_fe_set_fb_check.argtypes = [C.c_void_p, C.c_void_p]
    L.mskf_fe_get_fb_check.argtypes = [C.c_void_p, C.c_void_p]
    L.mskf_abi_version.restype = C.c_int
    assert L.mskf_abi_version() == 4
    syn = oracle.Synth(seed=0x5EED00D0, width=w, height=h)
    a, b = syn.render(0)
    s = _stream(gpu_ctx, oracle, w, h)
    assert s.get_fb_check() == (0, 1.0, 1.0)
    s.set_fb_check("temporal", 0.75, 2.5)
    held = (1, 0.75, 2.5)
    assert s.get_fb_check() == held
    nan, inf = float("nan"), float("inf")
    for bad in [FeFbCheck(4, 1, 1), FeFbCheck(7, 1, 1), FeFbCheck(-1, 1, 1), FeFbCheck(3, -0.001, 1), FeFbCheck(3, 1, 64.001), FeFbCheck(3, nan, 1), FeFbCheck(3, 1, nan),
                FeFbCheck(3, inf, 1), FeFbCheck(3, 1, -inf), FeFbCheck(0, 65.0, 1), FeFbCheck(0, 1, nan)]:
        assert L.mskf_fe_set_fb_check(s.h, C.byref(bad)) == -1 and len(L.mskf_last_error()) > 0
        assert s.get_fb_check() == held
    assert L.mskf_fe_set_fb_check(s.h, None) == -1 and L.mskf_fe_set_fb_check(None, None) == -1 and L.mskf_fe_get_fb_check(s.h, None) == -1
    assert _status(s.set_fb_check, "sometimes") == -1 and s.get_fb_check() == held
    for good in [(3, 0.0, 64.0), (3, 64.0, 0.0), (0, 0.0, 0.0), (2, 0.5, 0.5)]:          # the limits are accepted
        s.set_fb_check(*good)
        assert s.get_fb_check() == good
    s.set_fb_check(*held)
    # pending track batch
    s.push_stereo(a, b)
    pts = np.array([[40.0, 40.0], [90.0, 60.0]])
    gpu_ctx.track_batch_begin([s], [dict(pts=pts, do_temporal=0)])
    try:
        assert _status(s.set_fb_check, "both") == -1 and b"track batch" in L.mskf_last_error()
        assert _status(s.set_fb_check, "off") == -1
    finally:
        gpu_ctx.track_batch_end()
    assert s.get_fb_check() == held
    # a setting applies from the next call: threshold 0 on the stereo half removes matches that were there
    cm = s.cell_maxima()
    pts = np.stack([cm["x"], cm["y"]], 1)[cm["score"] > 2560][:120].astype(np.float32)
    r0 = s.track(pts, 0)
    s.set_fb_check("stereo", 1.0, 0.0)
    r1 = s.track(pts, 0)
    assert (r0["status"] == 3).sum() > 20 and (r1["status"] == 3).sum() < (r0["status"] == 3).sum()
    s.set_fb_check(*held)
    # pending device frame: refused, then accepted after its _end
    s.swap()
    s.set_grid()
    gpu_ctx.frame_batch_begin([s], [(a, b)], [{}])
    try:
        assert _status(s.set_fb_check, "both") == -1 and b"device frame" in L.mskf_last_error()
    finally:
        gpu_ctx.frame_batch_end()
    assert s.get_fb_check() == held
    s.set_fb_check("both")
    assert s.get_fb_check() == (3, 1.0, 1.0)
    s.set_fb_check("off")
    assert s.get_fb_check()[0] == 0
    s.close()


# ------------------------------------------------------------------------------------------ runners
_FB = dict(tt=0.004, ts=0.1)                  # tight enough that the clean synthetic sequence loses points to the check


def _check(r, stream=None):
    r.set_fb_check("both", _FB["tt"], _FB["ts"], stream=stream)


def _published_pass(frames, k, dump, before):
    """Every feature of frame k's dump passes the stereo half on frame k's images, and every one that frame k - 1 published too
    the temporal half against its pixel there."""
    ids, life, c0, c1 = dump[:4]
    a, b = frames[k]
    n = len(ids)
    p0, p1 = np.stack([c0["x"], c0["y"]], 1).astype(np.float32), np.stack([c1["x"], c1["y"]], 1).astype(np.float32)
    z = np.zeros((n, 2), np.float32)
    assert (FB.gate(None, a, b, FB.STEREO, _FB["tt"], _FB["ts"], 0, p0, p0, p1, z, z, np.full(n, 3, np.uint8))[4] == 3).all(), k
    n_tracked = 0
    if before is not None:
        was = {int(i): (x, y) for i, x, y in zip(before[0], before[2]["x"], before[2]["y"])}
        sel = np.array([int(i) in was for i in ids], bool)
        assert np.array_equal(sel, life > 1)
        pin = np.array([was[int(i)] for i in ids[sel]], np.float32).reshape(-1, 2)
        m = int(sel.sum())
        z = np.zeros((m, 2), np.float32)
        assert (FB.gate(frames[k - 1][0], a, None, FB.TEMPORAL, _FB["tt"], _FB["ts"], 1, pin, p0[sel], z, z, z, np.ones(m, np.uint8))[4] == 1).all(), k
        n_tracked = m
    return n_tracked


@_guarded
def test_runner_checked(oracle):
    """Every published feature of every frame passes the restatement recomputed from the frames, every frame after the first is
    a device frame; pipelined == lockstep == the frame-by-frame run, device books == host books, bit for bit; the check
    removes something; a second stream without the check is untouched."""
    w, h, n_frames = GP._RUN["w"], GP._RUN["h"], GP._RUN["n_frames"]
    syn = oracle.Synth(seed=GP._RUN["seed"], width=w, height=h)
    other = oracle.Synth(seed=GP._RUN["seed"] + 1, width=w, height=h)
    frames = [syn.render(k) for k in range(n_frames)]
    state = dict(before=None, tracked=0)

    def on_frame(k, d):
        assert len(d[0]) >= 1, k
        state["tracked"] += _published_pass(frames, k, d, state["before"])
        state["before"] = d
    _ok_to_launch()
    runs = GP._stepped_runs(syn, frames, _check, on_frame)          # (asserts device frames, and device books == host books)
    assert state["tracked"] > 5 * n_frames
    keep = []
    plain = GP._sequence_run(oracle, [syn, other], keep)
    for pipelined in (False, True):
        run = GP._sequence_run(oracle, [syn, other], keep, pipelined=pipelined, setup=lambda r: _check(r, stream=0))
        GP._same_run(run, runs[0])
        GP._same_run(run, plain, 1, 1)                      # the stream that does not check is untouched
        run.close()
    ids_p, ids_c = plain.dump(0)[0], runs[0].dump(0)[0]
    info_p, info_c = plain.dump(0)[4], runs[0].dump(0)[4]
    assert not np.array_equal(ids_p, ids_c) or (info_p.after_tracking, info_p.after_matching) != (info_c.after_tracking, info_c.after_matching)
    plain.close()
    for r in runs:
        r.close()


@_guarded
def test_runner_on_and_off_again_equals_never_on(oracle):
    syn = oracle.Synth(seed=GP._RUN["seed"], width=GP._RUN["w"], height=GP._RUN["h"])
    keep = []
    _ok_to_launch()
    plain = GP._sequence_run(oracle, [syn], keep)

    def on_off(r):
        _check(r)
        r.set_fb_check("off")
    off = GP._sequence_run(oracle, [syn], keep, setup=on_off)
    assert len(plain.dump(0)[0]) > 10
    GP._same_run(off, plain)
    for r in (plain, off):
        r.close()


@_guarded
def test_runner_set_fb_check_refuses_bad_arguments(oracle):
    from msckf_stereo_c_amd import runner as R
    _ok_to_launch()
    syn = oracle.Synth(seed=1, width=188, height=120)
    run = R.Runner(syn.calib, default_fe_cfg(), default_ekf_cfg(), 1, 2)
    for bad in [dict(mode="sometimes"), dict(mode=4), dict(max_error_temporal=64.5), dict(max_error_stereo=-0.5), dict(max_error_stereo=float("nan")),
                dict(max_error_temporal=float("inf")), dict(stream=2)]:
        with pytest.raises(capi.MskfError):
            run.set_fb_check(**bad)
    run.set_fb_check("stereo", stream=1)
    run.set_fb_check("off")
    run.close()


# ------------------------------------------------------------------------------------------ the app
@_guarded
def test_app_reads_fb_check_keys(tmp_path, oracle):
    """The headless app with the three fb_check keys in its app_imgproc.yaml logs the tracking counts of a Runner with the same
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
    tt, ts = 0.03125, 0.0625

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
    got_on, work, cfg = app("on", "fb_check: both\nfb_check_max_error_temporal: %r\nfb_check_max_error_stereo: %r\n" % (tt, ts))
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
            run.set_fb_check("both", tt, ts)
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
