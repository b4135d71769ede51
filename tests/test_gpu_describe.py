"""Opt-in 256-bit descriptors on the device (k_fe_describe; mskf_fe_describe*; ImageProcessor / Runner / the app) against the numpy
restatement of the contract (tests/brief_reference.py; DESIGN.md section 3, "Descriptors"), bit for bit: the kernel launched directly
with descriptors of the test's own between guard bytes (every size, the ones a stream refuses as too small included), the C ABI on
every role, push mode and option that changes level 0, batches, begin / end, every refusal, and the runners and the app."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import brief_cases as BC
import brief_reference as BR
from msckf_stereo_c_amd import capi
from msckf_stereo_c_amd.ctypes_types import FeDescribeArgs, default_ekf_cfg, default_fe_cfg

from hip_runtime import Hip

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 0xEE
_HIP_ERRORS = []                              # after a HIP error no test of this module launches anything


class FeDescribeDev(C.Structure):
    """FeDescribeDev of csrc/hip/fe_brief.h: one job of a launch."""
    _fields_ = [("img", C.c_void_p), ("w", C.c_int), ("h", C.c_int), ("pitch", C.c_longlong), ("pts", C.c_void_p), ("n", C.c_int), ("pad_", C.c_int),
                ("desc", C.c_void_p), ("valid", C.c_void_p)]


def test_fe_describe_dev_layout_matches_the_header(tmp_path):
    so = str(tmp_path / "libfe_brief_test.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-I", ROOT, "-o", so, os.path.join(ROOT, "tests", "cpp", "fe_brief_test.cpp")])
    out = (C.c_int * 16)()
    n = C.CDLL(so).fb_describe_dev_layout(out, 16)
    assert list(out[:n]) == [C.sizeof(FeDescribeDev)] + [getattr(FeDescribeDev, k).offset for k in ("img", "w", "h", "pitch", "pts", "n", "desc", "valid")]


# ------------------------------------------------------------------------------------------ the kernel, launched directly
def _launch(gpu_ctx, jobs, max_pts=None):
    """One fe_launch_describe over jobs = [(img, pitch or None, pts)].  Returns [(desc, valid)]; the guard bytes around every
    output array and the inputs are checked to be untouched."""
    assert not _HIP_ERRORS, "an earlier launch ended with a HIP error: %s" % _HIP_ERRORS
    f = gpu_ctx.L.fe_launch_describe
    f.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    f.restype = None
    hip = Hip()
    try:
        bufs, img_off, pts_off, out_off = [], [], [], []
        n_img = 64
        for img, pitch, pts in jobs:
            h, w = img.shape
            b = np.ascontiguousarray(img) if pitch is None else BC.padded(img, pitch)
            assert w >= 1 and h >= 1 and b.shape[1] >= w                    # what keeps every read of the kernel inside the buffer
            bufs.append(b)
            img_off.append(n_img)
            n_img += b.size + 64
        host_img = np.full(n_img, 0xA5, np.uint8)
        for b, o in zip(bufs, img_off):
            host_img[o:o + b.size] = b.reshape(-1)
        n_pts = 0
        for _, _, pts in jobs:
            pts_off.append(n_pts)
            n_pts += len(pts)
        host_pts = np.zeros((max(n_pts, 1), 2), np.float32)
        for (_, _, pts), o in zip(jobs, pts_off):
            host_pts[o:o + len(pts)] = pts
        # outputs: guard, desc (32 n), guard, valid (n), guard; the guards are 13 bytes, so nothing is aligned
        n_out = 13
        for _, _, pts in jobs:
            n = len(pts)
            out_off.append((n_out, n_out + 32 * n + 13))
            n_out += 32 * n + 13 + n + 13
        host_out = np.full(n_out, GUARD, np.uint8)
        d_img, d_pts, d_out = hip.alloc(n_img, False), hip.alloc(host_pts.nbytes, False), hip.alloc(n_out, False)
        hip.put(d_img, host_img)
        hip.put(d_pts, host_pts)
        hip.put(d_out, host_out)
        desc = (FeDescribeDev * len(jobs))()
        for d, b, (img, _, pts), io, po, (do, vo) in zip(desc, bufs, jobs, img_off, pts_off, out_off):
            d.img, d.w, d.h, d.pitch = d_img + io, img.shape[1], img.shape[0], b.shape[1]
            d.pts, d.n = d_pts + 8 * po, len(pts)
            d.desc, d.valid = d_out + do, d_out + vo
        raw = np.frombuffer(bytes(desc), np.uint8).copy()
        d_desc = hip.alloc(raw.size, False)
        hip.put(d_desc, raw)
        f(d_desc, len(jobs), max((len(p) for _, _, p in jobs), default=0) if max_pts is None else max_pts, gpu_ctx.hip_stream())
        gpu_ctx.sync()
        err = hip.last_error()
        assert err == 0, "hipGetLastError %d after k_fe_describe" % err
        got = hip.get(d_out, n_out)
        assert np.array_equal(hip.get(d_img, n_img), host_img) and np.array_equal(hip.get(d_pts, host_pts.nbytes).view(np.float32).reshape(-1, 2), host_pts, equal_nan=True)
    except BaseException as e:
        _HIP_ERRORS.append(repr(e))
        raise
    finally:
        hip.free()
    inside = np.zeros(n_out, bool)
    res = []
    for (_, _, pts), (do, vo) in zip(jobs, out_off):
        n = len(pts)
        inside[do:do + 32 * n] = True
        inside[vo:vo + n] = True
        res.append((got[do:do + 32 * n].reshape(n, 32), got[vo:vo + n]))
    assert np.all(got[~inside] == GUARD), "a byte landed outside the output arrays"
    return res


def _same(got, want, what):
    assert np.array_equal(got[1], want[1]), (what, "valid", np.flatnonzero(got[1] != want[1])[:8])
    assert np.array_equal(got[0], want[0]), (what, "desc", np.flatnonzero((got[0] != want[0]).any(axis=1))[:8])


@pytest.mark.parametrize("size", BC.SIZES, ids=lambda s: "%dx%d" % s)
def test_direct_every_kind(gpu_ctx, size):
    """The lattice, the border centres and the validity edges of one size on every image kind, a job each, in one launch."""
    w, h = size
    pts = BC.points(w, h)
    jobs = [(BC.image(kind, w, h), BC.PITCH.get(size), pts) for kind in BC.KINDS]
    for kind, got, (img, _, _) in zip(BC.KINDS, _launch(gpu_ctx, jobs), jobs):
        want = BR.describe(img, pts)
        _same(got, want, (size, kind))
        assert 0 < want[1].sum() < len(pts)


@pytest.mark.parametrize("n", BC.COUNTS)
def test_direct_point_counts(gpu_ctx, n):
    jobs = [(BC.image("random", w, h), BC.PITCH.get((w, h)), BC.counted_points(w, h, n)) for (w, h) in [(30, 31), (129, 71)]]
    for got, (img, _, pts) in zip(_launch(gpu_ctx, jobs), jobs):
        assert got[1].shape == (n,)
        _same(got, BR.describe(img, pts), n)


def test_direct_known_answers(gpu_ctx):
    yy, xx = np.mgrid[0:60, 0:60]
    flat, white, one = np.full((40, 50), 131, np.uint8), np.full((40, 50), 255, np.uint8), np.array([[77]], np.uint8)
    p = np.array([[25, 20], [0, 0], [49, 39], [-0.5, 39.4], [50, 20], [np.nan, 3]], np.float32)
    c = np.array([[30, 30]], np.float32)
    got = _launch(gpu_ctx, [(flat, None, p), (white, None, p), (one, None, np.array([[0, 0], [-0.5, 0.25], [0.5, 0]], np.float32)),
                            ((4 * xx).astype(np.uint8), None, c), ((4 * yy).astype(np.uint8), None, c)])
    for k in (0, 1):
        assert got[k][1].tolist() == [1, 1, 1, 1, 0, 0] and not got[k][0].any()
    assert got[2][1].tolist() == [1, 1, 0] and not got[2][0].any()
    bits = [np.unpackbits(g[0], axis=1, bitorder="little")[0] for g in got[3:]]
    assert np.array_equal(bits[0], BR.PATTERN[:, 0] < BR.PATTERN[:, 2]) and np.array_equal(bits[1], BR.PATTERN[:, 1] < BR.PATTERN[:, 3])


MIXED = [((333, 251), "smooth", 257), ((1, 1), "random", 5), ((64, 64), "blocks", 64), ((5, 3), "random", 63), ((129, 71), "edges", 65), ((29, 29), "checker1", 1),
         ((30, 31), "random", 200), ((64, 64), "random", 0), ((129, 71), "random", 129), ((333, 251), "blocks", 31), ((30, 31), "edges", 2)]


def test_direct_eleven_jobs_in_one_launch(gpu_ctx):
    """Eleven jobs of different sizes and counts (one of them empty, between two others) in one launch cut for the largest; and
    the same jobs in a launch cut for fewer points than the largest job has: a workgroup then takes several points."""
    assert len(MIXED) == 11
    jobs = [(BC.image(kind, w, h), BC.PITCH.get((w, h)), BC.counted_points(w, h, n, seed=k)) for k, ((w, h), kind, n) in enumerate(MIXED)]
    want = [BR.describe(img, pts) for img, _, pts in jobs]
    for max_pts in (None, 40):
        for k, (got, w_) in enumerate(zip(_launch(gpu_ctx, jobs, max_pts), want)):
            _same(got, w_, (MIXED[k], max_pts))
    assert want[7][0].shape == (0, 32)


def test_direct_nothing_to_do(gpu_ctx):
    """No job, and jobs without points: no launch, nothing written."""
    img = BC.image("random", 30, 31)
    none = np.zeros((0, 2), np.float32)
    assert _launch(gpu_ctx, [(img, None, none), (img, None, none)])[1][0].shape == (0, 32)


# ------------------------------------------------------------------------------------------ through the C ABI
def _stream(ctx, oracle, w, h):
    return capi.Stream(ctx, oracle.euroc_calib(w, h), default_fe_cfg(), default_ekf_cfg())


def _pair(w, h, k=0):
    return BC.image("blocks", w, h, seed=20 + 2 * k), BC.image("smooth", w, h, seed=21 + 2 * k)


def _status(call, *a, **kw):
    try:
        call(*a, **kw)
        return 0
    except capi.MskfError as e:
        return e.code


def _check_role(s, role, pts, image=None):
    """describe(role) == the restatement on get_level(role, 0) (== `image` when given)."""
    lvl = s.get_level(role, 0)
    if image is not None:
        assert np.array_equal(lvl, image), role
    got = s.describe(role, pts)
    _same(got, BR.describe(lvl, pts), ("role", role))
    return got


ABI_SIZES = [(64, 64), (129, 71), (752, 480)]


@pytest.mark.parametrize("w,h", ABI_SIZES)
def test_abi_roles(gpu_ctx, oracle, w, h):
    """Roles 0, 1 and 2 after one push, after push + swap + push, and after a device frame."""
    pts = BC.points(w, h)
    (a0, b0), (a1, b1), (a2, b2) = _pair(w, h, 0), _pair(w, h, 1), _pair(w, h, 2)
    L = gpu_ctx.L
    s = _stream(gpu_ctx, oracle, w, h)
    for role in (0, 1, 2):
        assert _status(s.describe, role, pts) == -1 and b"describe" in L.mskf_last_error()       # nothing pushed
    s.push_stereo(a0, b0)
    _check_role(s, 1, pts, a0)
    _check_role(s, 2, pts, b0)
    assert _status(s.describe, 0, pts) == -1 and b"no previous image" in L.mskf_last_error()
    s.swap()
    _check_role(s, 0, pts, a0)
    assert _status(s.describe, 1, pts) == -1 and b"no stereo pair pushed yet" in L.mskf_last_error()
    s.push_stereo(a1, b1)
    d0, d1, d2 = _check_role(s, 0, pts, a0), _check_role(s, 1, pts, a1), _check_role(s, 2, pts, b1)
    assert not np.array_equal(d0[0], d1[0]) and not np.array_equal(d1[0], d2[0])
    if w == 752:
        assert s.grid_capacity() > 0
    if s.grid_capacity() > 0:
        s.swap()
        s.set_grid()
        gpu_ctx.frame_batch_begin([s], [(a2, b2)], [{}])
        gpu_ctx.frame_batch_end()
        # (the frame has rotated the pyramids: its cam0 is now the previous image, role 1 holds the image before it)
        _check_role(s, 0, pts, a2)
        _check_role(s, 2, pts, b2)
        _check_role(s, 1, pts, a1)
    s.close()


def test_abi_push_modes(gpu_ctx, oracle):
    """A host push with padded rows, a device push (copied) and a borrowed device push (read in place, at an unaligned address)."""
    w, h = 129, 71
    pts = BC.points(w, h)
    a, b = _pair(w, h)
    want = (BR.describe(a, pts), BR.describe(b, pts))
    s = _stream(gpu_ctx, oracle, w, h)
    pa, pb = BC.padded(a, 141), BC.padded(b, 141)          # (named: the push reads them when the stream gets there)
    s.push_stereo(pa, pb, pitch=141)
    _same(_check_role(s, 1, pts, a), want[0], "pitched")
    _same(_check_role(s, 2, pts, b), want[1], "pitched")
    s.close()
    hip = Hip()
    try:
        host = [np.full(256 + w * h + 256, 0xC3, np.uint8) for _ in range(2)]
        host[0][131:131 + w * h], host[1][144:144 + w * h] = a.reshape(-1), b.reshape(-1)
        dev = [hip.alloc(x.size, False) for x in host]
        for d, x in zip(dev, host):
            hip.put(d, x)
        for on_device in (1, 2):
            s = _stream(gpu_ctx, oracle, w, h)
            gpu_ctx.push_stereo_batch([s], [dev[0] + 131], [dev[1] + 144], on_device=on_device)
            _same(_check_role(s, 1, pts, a), want[0], on_device)
            _same(_check_role(s, 2, pts, b), want[1], on_device)
            for d, x in zip(dev, host):
                assert np.array_equal(hip.get(d, x.size), x)
            s.close()
    finally:
        hip.free()


def test_abi_options_that_change_level0(gpu_ctx, oracle):
    """CLAHE on: the equalised plane is described; a GRAY16 input: the converted plane; a mask does not enter."""
    w, h = 129, 71
    pts = BC.points(w, h)
    a, b = _pair(w, h)
    plain = (BR.describe(a, pts), BR.describe(b, pts))
    s = _stream(gpu_ctx, oracle, w, h)
    s.set_equalize("clahe", (4, 3), 3.0)
    s.push_stereo(a, b)
    got = _check_role(s, 1, pts)
    assert not np.array_equal(s.get_level(1, 0), a) and got[1].any()
    _check_role(s, 2, pts)
    s.close()
    s = _stream(gpu_ctx, oracle, w, h)
    s.set_input_format("gray16", 4)
    a16, b16 = (a.astype(np.uint16) << 4) | 9, (b.astype(np.uint16) << 4) | 3
    s.push_stereo(a16, b16)
    _same(_check_role(s, 1, pts, a), plain[0], "gray16")
    _same(_check_role(s, 2, pts, b), plain[1], "gray16")
    s.close()
    s = _stream(gpu_ctx, oracle, w, h)
    m = np.ones((h, w), np.uint8)
    m[:, : w // 2] = 0
    s.set_mask(cam0=m, cam1=m, margin=3)
    s.push_stereo(a, b)
    _same(_check_role(s, 1, pts, a), plain[0], "masked")
    _same(_check_role(s, 2, pts, b), plain[1], "masked")
    s.close()


def test_abi_batches_equal_single_calls(gpu_ctx, oracle):
    """Batches of 1, 2, 3 and 5 streams of three sizes with empty members == the single calls; begin / end with host work (and a
    push of another stream) between == the same; an all-empty batch leaves nothing pending."""
    shapes = [(64, 64), (129, 71), (188, 120), (129, 71), (64, 64)]
    streams, imgs = [], []
    for k, (w, h) in enumerate(shapes):
        s = _stream(gpu_ctx, oracle, w, h)
        a, b = _pair(w, h, k)
        s.push_stereo(a, b)
        streams.append(s)
        imgs.append((a, b))
    roles = [1, 2, 1, 2, 1]
    counts = [65, 0, 257, 1, 0]
    pts = [BC.counted_points(w, h, n, seed=k) for k, ((w, h), n) in enumerate(zip(shapes, counts))]
    single = [s.describe(r, p) for s, r, p in zip(streams, roles, pts)]
    for k, (g, (a, b), r, p) in enumerate(zip(single, imgs, roles, pts)):
        _same(g, BR.describe(a if r == 1 else b, p), ("single", k))
    for sel in ([0], [1, 2], [0, 1, 2], [2, 1, 0], [0, 1, 2, 3, 4]):
        got = gpu_ctx.describe_batch([streams[i] for i in sel], [roles[i] for i in sel], [pts[i] for i in sel])
        for i, g in zip(sel, got):
            _same(g, single[i], ("batch", sel, i))
    # an all-empty batch: OK, nothing pending (a describe call right after it is not refused)
    none = [None, None]
    out = gpu_ctx.describe_batch_begin(streams[:2], [1, 1], none)
    assert [o[0].shape for o in out] == [(0, 32), (0, 32)]
    got = gpu_ctx.describe_batch_begin(streams, roles, pts)
    # between begin and end: host work, and a push of one of the streams (it runs behind the describe launch)
    a_new, b_new = _pair(*shapes[0], 9)
    want_new = BR.describe(a_new, pts[0])
    streams[0].push_stereo(a_new, b_new)
    gpu_ctx.describe_batch_end()
    for i, g in enumerate(got):
        _same(g, single[i], ("begin / end", i))
    _same(streams[0].describe(1, pts[0]), want_new, "after the push")
    gpu_ctx.describe_batch_end()             # nothing pending: a no-op
    for s in streams:
        s.close()


def test_abi_refusals(gpu_ctx, oracle):
    """Every refusal is MSKF_ERR_INVALID with a reason, touches nothing and leaves the stream usable."""
    w, h = 64, 64
    L = gpu_ctx.L
    L.mskf_fe_describe.argtypes = [C.c_void_p, C.c_void_p]
    L.mskf_fe_describe_batch.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    a, b = _pair(w, h)
    pts = BC.counted_points(w, h, 65)
    want = BR.describe(a, pts)
    s = _stream(gpu_ctx, oracle, w, h)
    s.push_stereo(a, b)
    _same(s.describe(1, pts), want, "before")

    def refused(rc, text):
        assert rc == -1 and text in L.mskf_last_error(), (rc, L.mskf_last_error())
        _same(s.describe(1, pts), want, text)

    p = np.ascontiguousarray(pts)
    desc, valid = np.full((len(p), 32), GUARD, np.uint8), np.full(len(p), GUARD, np.uint8)

    def args(role=1, n=len(p), pts_=p.ctypes.data, desc_=desc.ctypes.data, valid_=valid.ctypes.data):
        return FeDescribeArgs(role, n, pts_, desc_, valid_)
    hs = (C.c_void_p * 1)(s.h)
    refused(L.mskf_fe_describe(None, C.byref(args())), b"null argument")
    refused(L.mskf_fe_describe(s.h, None), b"null argument")
    refused(L.mskf_fe_describe_batch(gpu_ctx.h, 1, None, C.byref(args())), b"null argument")
    refused(L.mskf_fe_describe_batch(gpu_ctx.h, 1, hs, None), b"null argument")
    refused(L.mskf_fe_describe_batch(None, 1, hs, C.byref(args())), b"null argument")
    refused(L.mskf_fe_describe_batch(gpu_ctx.h, 1, (C.c_void_p * 1)(None), C.byref(args())), b"null stream")
    for role in (-1, 3):
        refused(L.mskf_fe_describe(s.h, C.byref(args(role=role))), b"role must be")
    refused(L.mskf_fe_describe(s.h, C.byref(args(role=0))), b"no previous image")
    refused(L.mskf_fe_describe(s.h, C.byref(args(n=-1))), b"negative point count")
    refused(L.mskf_fe_describe(s.h, C.byref(args(pts_=None))), b"null pts, desc or valid")
    refused(L.mskf_fe_describe(s.h, C.byref(args(desc_=None))), b"null pts, desc or valid")
    refused(L.mskf_fe_describe(s.h, C.byref(args(valid_=None))), b"null pts, desc or valid")
    assert (desc == GUARD).all() and (valid == GUARD).all()
    # a stream of another context (the second member of a batch: the first is not touched either)
    other = capi.Context(0)
    s2 = _stream(other, oracle, w, h)
    s2.push_stereo(a, b)
    refused(_status(gpu_ctx.describe_batch, [s, s2], [1, 1], [pts, pts]), b"another context")
    _same(s2.describe(2, pts), BR.describe(b, pts), "the other context's stream")
    s2.close()
    other.close()
    # while a track batch, a device frame or a describe batch of the context is pending
    t = _stream(gpu_ctx, oracle, 188, 120)
    ta, tb = _pair(188, 120)
    t.push_stereo(ta, tb)
    gpu_ctx.track_batch_begin([t], [dict(pts=np.array([[30, 30]], np.float32), do_temporal=0)])
    assert _status(s.describe, 1, pts) == -1 and b"track batch" in L.mskf_last_error()
    gpu_ctx.track_batch_end()
    _same(s.describe(1, pts), want, "after the track batch")
    assert t.grid_capacity() > 0
    t.swap()
    t.set_grid()
    gpu_ctx.frame_batch_begin([t], [(ta, tb)], [{}])
    assert _status(s.describe, 1, pts) == -1 and b"device frame" in L.mskf_last_error()
    gpu_ctx.frame_batch_end()
    _same(s.describe(1, pts), want, "after the device frame")
    got = gpu_ctx.describe_batch_begin([s], [1], [pts])
    assert _status(t.describe, 2, pts) == -1 and b"describe batch" in L.mskf_last_error()
    gpu_ctx.describe_batch_end()
    _same(got[0], want, "the pending batch itself")
    _same(s.describe(1, pts), want, "after everything")
    t.close()
    s.close()


# ------------------------------------------------------------------------------------------ runners
_RUN = dict(w=188, h=120, n_frames=30)          # (25 static frames, then the camera moves: the filter publishes poses)


def _msg_bytes(m):
    """The records of a message without their padding bytes (which nothing defines)."""
    return b"".join(np.ascontiguousarray(m[k]).tobytes() for k in ("id", "u0", "v0", "u1", "v1"))


def _pixels(c0):
    return np.stack([c0["x"], c0["y"]], axis=1).astype(np.float32)


def _step_all(runs, syns, n_frames, each_frame):
    j = 0
    for k in range(n_frames):
        t_img = syns[0].frame_time(k)
        while True:
            smp = [syn.imu(j) for syn in syns]
            j += 1
            for r in runs:
                for i, s in enumerate(smp):
                    r.imu(i, s)
            if not (smp[0].time_stamp <= t_img):
                break
        frames = [syn.render(k) for syn in syns]
        for r in runs:
            r.step([f[0] for f in frames], [f[1] for f in frames], [t_img] * len(syns))
        each_frame(k, frames)


def test_runner_descriptors(oracle):
    """Two streams, stream 0 describing: Runner.descriptors of every frame (the phased first frame included) == the restatement on
    that frame's cam0 image at the published cam0 pixels, ids aligned with msg; device books == host books; the messages and poses of
    both streams are those of a run with descriptors off, bit for bit; the other stream returns empty arrays."""
    from msckf_stereo_c_amd import runner as R
    w, h, n_frames = _RUN["w"], _RUN["h"], _RUN["n_frames"]
    syns = [oracle.Synth(seed=0x5EED00D0 + i, width=w, height=h) for i in range(2)]
    fe, ekf = default_fe_cfg(), default_ekf_cfg(max_cam_state_size=10)
    on, off, host = (R.Runner(syns[0].calib, fe, ekf, 1, 2) for _ in range(3))
    on.set_descriptors(True, stream=0)
    host.set_descriptors(True)
    host.set_descriptors(False, stream=1)
    seen = []

    def each_frame(k, frames):
        ids, desc, valid = on.descriptors(0)
        d_ids, _, c0, _, _ = on.dump(0)
        assert len(ids) == len(d_ids) >= 1 and np.array_equal(ids, d_ids), k
        assert np.array_equal(on.msg(0)["id"][:len(ids)], ids.astype(on.msg(0)["id"].dtype)), k
        want = BR.describe(frames[0][0], _pixels(c0))
        _same((desc, valid), want, ("frame", k))
        assert valid.all(), k
        for x in on.descriptors(1):
            assert x.shape[0] == 0
        seen.append((ids, desc))
        for i in range(2):
            assert _msg_bytes(on.msg(i)) == _msg_bytes(off.msg(i)), (k, i)
    try:
        # (the switch is process-wide: the host-books runner steps on its own)
        _step_all([on, off], syns, n_frames, each_frame)
        assert on.num_device_frames(0) == n_frames - 1
        R.set_fe_books_on_host(1)
        k_host = []

        def each_host(k, frames):
            ids, desc, valid = host.descriptors(0)
            assert np.array_equal(ids, seen[k][0]) and np.array_equal(desc, seen[k][1]) and valid.all(), k
            k_host.append(k)
        _step_all([host], syns, n_frames, each_host)
        assert host.num_device_frames(0) == 0 and len(k_host) == n_frames
    finally:
        R.set_fe_books_on_host(-1)
    for i in range(2):
        pa, pb = on.poses(i), off.poses(i)
        assert len(pa) == len(pb) > 3 and pa.tobytes() == pb.tobytes()
    # a feature keeps its descriptor, nearly: the same id in consecutive frames is much closer than different ids
    (i0, d0), (i1, d1) = seen[-2], seen[-1]
    common = np.intersect1d(i0, i1)
    assert len(common) >= 5
    a = np.array([d0[np.flatnonzero(i0 == c)[0]] for c in common])
    b = np.array([d1[np.flatnonzero(i1 == c)[0]] for c in common])
    assert np.median(BR.hamming(a, b)) < np.median(BR.hamming(a[:, None, :], b[None, :, :])[~np.eye(len(common), dtype=bool)]) / 2
    # turned off again: empty arrays from the next frame on
    on.set_descriptors(False)
    assert on.descriptors(0)[0].shape[0] == 0
    for r in (on, off, host):
        r.close()


def test_runner_pipelined_equals_lockstep(oracle):
    from msckf_stereo_c_amd import runner as R
    from test_gpu_system import _attach_sequences
    w, h, n_frames = _RUN["w"], _RUN["h"], _RUN["n_frames"]
    syns = [oracle.Synth(seed=0x5EED00D0 + i, width=w, height=h) for i in range(2)]
    keep, res = [], []
    for pipelined in (False, True):
        run = R.Runner(syns[0].calib, default_fe_cfg(), default_ekf_cfg(max_cam_state_size=10), 1, 2, host_threads=1)
        run.set_descriptors(True, stream=0)
        _attach_sequences(oracle, run, syns, n_frames, keep)
        run.run(0, n_frames, threaded=True, pipelined=pipelined)
        ids, desc, valid = run.descriptors(0)
        d_ids, _, c0, _, _ = run.dump(0)
        assert np.array_equal(ids, d_ids) and len(ids) >= 1 and run.descriptors(1)[0].shape[0] == 0
        _same((desc, valid), BR.describe(syns[0].render(n_frames - 1)[0], _pixels(c0)), pipelined)
        assert len(run.poses(0)) > 3
        res.append((ids, desc, valid, run.poses(0).tobytes(), run.poses(1).tobytes(), _msg_bytes(run.msg(0)), _msg_bytes(run.msg(1))))
        run.close()
    for k, (x, y) in enumerate(zip(*res)):
        assert np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y, k


# ------------------------------------------------------------------------------------------ the app
def test_app_writes_descriptors_out(tmp_path, oracle):
    """The headless app with descriptors_out in its app_imgproc.yaml writes one line per feature and frame, "time id hex", whose
    ids and hex digits are those of a Runner of one on the same files."""
    import shutil
    from PIL import Image
    from msckf_stereo_c_amd import build
    from msckf_stereo_c_amd import runner as R
    from msckf_stereo_c_amd.ctypes_types import Calib, EkfCfg, FeCfg, ImuSample
    build.build_all()
    n_frames, w, h = 6, 752, 480
    syn = oracle.Synth(seed=0x5EED0042, width=w, height=h)
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
        Image.fromarray(a).save(mav0 / "cam0" / "data" / name)
        Image.fromarray(b).save(mav0 / "cam1" / "data" / name)
        rows.append("%d,%s\r" % (t0_ns + k * dt_ns, name))
    for c in (0, 1):
        (mav0 / ("cam%d" % c) / "data.csv").write_text("#timestamp [ns],filename\r\n" + "\n".join(rows) + "\n")
    lines = ["#timestamp [ns],w_x,w_y,w_z,a_x,a_y,a_z"]
    for j in range((n_frames + 2) * 10):
        s = syn.imu(j)
        vals = list(s.angular_velocity) + list(s.linear_acceleration)
        lines.append("%d,%s" % (t0_ns + j * (dt_ns // 10), ",".join("%.9g" % v for v in vals)))
    (mav0 / "imu0" / "data.csv").write_text("\n".join(lines) + "\n")
    cfg = tmp_path / "config"
    shutil.copytree(os.path.join(ROOT, "config"), cfg)
    with open(cfg / "app_imgproc.yaml", "a") as f:
        f.write("\ndescriptors: brief256\ndescriptors_out: descriptors_out.txt\n")
    work = tmp_path / "build"
    work.mkdir()
    exe = os.path.join(ROOT, "msckf_stereo_c_amd", "_build", "run_euroc_single_thread")
    res = subprocess.run([exe, str(mav0)], cwd=work, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    got = [line.split() for line in (work / "descriptors_out.txt").read_text().strip().splitlines()]
    assert all(len(g) == 3 and len(g[2]) == 64 for g in got)

    def stamp(ns):          # what the app parses: seconds * 1e9 + nanoseconds in double
        return (int(str(ns)[:-9]) * 1e9 + int(str(ns)[-9:])) * 1e-9
    imu = []
    for line in lines[1:]:
        f = line.split(",")
        v = [float(np.float32(x)) for x in f[1:7]]
        imu.append(ImuSample(stamp(int(f[0])), (C.c_double * 3)(*v[:3]), (C.c_double * 3)(*v[3:])))
    calib, fe, ekf = Calib(), FeCfg(), EkfCfg()
    assert R.lib().mskfh_load_configs(str(cfg).encode(), C.byref(calib), C.byref(fe), C.byref(ekf)) == 0
    run = R.Runner(calib, fe, ekf, 1, 1)
    run.set_descriptors(True)
    view = R.StreamView(run)
    want, j = [], 0
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
        ids, desc, valid = run.descriptors(0)
        assert len(ids) >= 1 and valid.all()
        want += [("%.9f" % t_img, str(int(i)), bytes(d).hex()) for i, d in zip(ids, desc)]
    run.close()
    assert len(got) == len(want)
    assert [tuple(g) for g in got] == want
