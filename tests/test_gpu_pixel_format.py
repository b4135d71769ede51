"""Input pixel formats of a stream on the device (mskf_fe_set_input_format; k_px_convert) against the numpy restatement of the
contract (tests/pixel_format_reference.py), bit for bit."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import equalize_reference as ER
import pixel_format_reference as PR
from msckf_stereo_c_amd import capi
from msckf_stereo_c_amd.ctypes_types import default_ekf_cfg, default_fe_cfg

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONVERTING = [n for n in PR.FORMATS if n != "gray8"]
SIZES = [(16, 16), (40, 24), (67, 45), (188, 120), (333, 251), (1024, 64)]       # w, h


def _shifts(fmt):
    return (0, 4, 8) if fmt == "gray16" else (0,)


def _stream(ctx, oracle, w, h, fmt=None, shift=0):
    s = capi.Stream(ctx, oracle.euroc_calib(w, h), default_fe_cfg(), default_ekf_cfg())
    if fmt is not None:
        s.set_input_format(fmt, shift)
    return s


def _pair(w, h, fmt, k=0, shift=0):
    """Two different raw images of the shared set (the kinds rotate with k)."""
    imgs = PR.raw_images(w, h, fmt, seed=k, shift=shift)
    return imgs[PR.KINDS[k % 8]], imgs[PR.KINDS[(k + 3) % 8]]


def _levels(s, roles=(1, 2)):
    return [s.get_level(role, l) for role in roles for l in range(4)]


def _same(a, b):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), (i, int((x != y).sum()) if x.shape == y.shape else None)


class _Dev:
    """A device buffer holding a copy of a host array, through the HIP runtime the product library itself is linked against."""

    def __init__(self, arr):
        self.L = capi.lib()
        self.host = np.ascontiguousarray(arr)
        self.p = C.c_void_p()
        self.L.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        self.L.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        self.L.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
        self.L.hipFree.argtypes = [C.c_void_p]
        assert self.L.hipMalloc(C.byref(self.p), self.host.nbytes) == 0
        assert self.L.hipMemcpy(self.p, self.host.ctypes.data, self.host.nbytes, 1) == 0

    def data_ptr(self):
        return self.p.value

    def read(self):
        out = np.empty_like(self.host)
        assert self.L.hipMemcpy(out.ctypes.data, self.p, out.nbytes, 2) == 0
        return out

    def zero(self):
        assert self.L.hipMemset(self.p, 0, self.host.nbytes) == 0
        assert self.L.hipDeviceSynchronize() == 0

    def __del__(self):
        if self.p:
            self.L.hipFree(self.p)
            self.p = None


PxJob = PR.PxJob          # the ctypes mirror of PxJob (checked against the header in test_pixel_format_reference.py)


def _launch_direct(ctx, jobs):
    """k_px_convert over bare images, as a converting push enqueues it (fe_launch_px_convert), for sizes and alignments no
    stream can have.  jobs: dicts(raw, fmt, shift, pad, src_off, dst_off).  Every source sits src_off bytes into a buffer and
    is cut after the last pixel of its last row (no padding behind it), canaries either side; every destination sits dst_off
    bytes into a canary buffer.  Returns the outputs; checks that the sources and
    all canaries are untouched."""
    recs, keep = (PxJob * len(jobs))(), []
    max_w = max_h = 0
    for r, j in zip(recs, jobs):
        name = PR.name_of(j["fmt"])
        rows = PR.raw_bytes(j["raw"], name, j.get("pad", 0))
        h, w = j["raw"].shape[:2]
        pitch = rows.shape[1]
        used = (h - 1) * pitch + w * PR.BPP[name]              # the bytes the kernel may read
        s_off, d_off = 64 + j.get("src_off", 0), 64 + j.get("dst_off", 0)
        host = np.full(s_off + used + 64, 0xA5, np.uint8)
        host[s_off:s_off + used] = rows.reshape(-1)[:used]
        src = _Dev(host)
        dhost = np.full(d_off + w * h + 64, 0x5A, np.uint8)
        dst = _Dev(dhost)
        r.src, r.dst, r.pitch = src.data_ptr() + s_off, dst.data_ptr() + d_off, pitch
        r.w, r.h, r.format, r.shift = w, h, PR.FORMATS[name], j.get("shift", 0)
        max_w, max_h = max(max_w, w), max(max_h, h)
        keep.append((src, host, dst, dhost, d_off, w, h))
    recs_dev = _Dev(np.frombuffer(bytes(recs), np.uint8).copy())
    f = ctx.L.fe_launch_px_convert
    f.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    f.restype = None
    f(recs_dev.data_ptr(), len(jobs), max_w, max_h, ctx.hip_stream())
    ctx.sync()
    outs = []
    for src, host, dst, dhost, d_off, w, h in keep:
        assert np.array_equal(src.read(), host)
        d = dst.read()
        outs.append(d[d_off:d_off + w * h].reshape(h, w).copy())
        d[d_off:d_off + w * h] = 0x5A
        assert np.array_equal(d, dhost)
    return outs


@pytest.mark.parametrize("fmt,w,h", [(f, w, h) for f in CONVERTING for w, h in SIZES] + [("rgb8", 752, 480), ("bayer_grbg8", 752, 480)])
def test_converted_level0_and_pyramid_bit_exact(gpu_ctx, oracle, fmt, w, h):
    """Level 0 of both cameras after a converting push == the restatement; levels 1 .. 3 and the cell maxima == those of a
    GRAY8 stream that was pushed the restatement's output.  mskf_stream_create refuses images under 64 pixels in a dimension,
    so 16 x 16 (a row is one chunk), 40 x 24 and 67 x 45 run the same kernel over bare images through fe_launch_px_convert, in
    one batch, dense and pitched, at aligned and unaligned addresses."""
    even = 2 if fmt == "gray16" else 1           # 16-bit pixels sit on 2-byte boundaries
    if w < 64 or h < 64:
        jobs, want = [], []
        for shift in _shifts(fmt):
            for n, raw in enumerate(_pair(w, h, fmt, shift, shift)):
                for pad, src_off, dst_off in ((0, 0, 0), (6, 5 * even, 0), (0, 3 * even, 16), (6, 0, 7 + n)):
                    jobs.append(dict(raw=raw, fmt=fmt, shift=shift, pad=pad, src_off=src_off, dst_off=dst_off))
                    want.append(PR.convert(raw, fmt, shift))
        _same(_launch_direct(gpu_ctx, jobs), want)
        return
    plain = _stream(gpu_ctx, oracle, w, h)
    for k, shift in enumerate(_shifts(fmt)):
        s = _stream(gpu_ctx, oracle, w, h, fmt, shift)
        assert s.get_input_format() == (PR.FORMATS[fmt], shift)
        a, b = _pair(w, h, fmt, k + 1, shift)
        s.push_stereo(a, b)
        ca, cb = PR.convert(a, fmt, shift), PR.convert(b, fmt, shift)
        assert np.array_equal(s.get_level(1, 0), ca), (shift, "cam0")
        assert np.array_equal(s.get_level(2, 0), cb), (shift, "cam1")
        maxima = s.cell_maxima()
        plain.push_stereo(ca, cb)
        assert maxima.tobytes() == plain.cell_maxima().tobytes()
        _same(_levels(s), _levels(plain))
        plain.swap()
        s.close()
    plain.close()


def test_bare_images_at_unaligned_planes(gpu_ctx):
    """The kernel's own edges at a ragged size a stream could have: destination planes at every offset 1 .. 15 from a 16-byte
    boundary (row starts then walk through all alignments: the byte-by-byte ends), sources at odd addresses, padded rows."""
    w, h = 203, 77
    jobs, want = [], []
    for k, fmt in enumerate(CONVERTING):
        even = 2 if fmt == "gray16" else 1
        raw = _pair(w, h, fmt, k, 4)[0]
        for dst_off in (1 + k, 15 - k):
            jobs.append(dict(raw=raw, fmt=fmt, shift=4 if fmt == "gray16" else 0, pad=6 * (dst_off & 1), src_off=even * (3 + k), dst_off=dst_off))
            want.append(PR.convert(raw, fmt, 4 if fmt == "gray16" else 0))
    _same(_launch_direct(gpu_ctx, jobs), want)


def _canary_buffer(rows, offset):
    host = np.full(256 + rows.size + 256, 0xC3, np.uint8)
    host[offset:offset + rows.size] = rows.reshape(-1)
    return host, _Dev(host)


@pytest.mark.parametrize("fmt,shift", [("gray16", 4), ("rgb8", 0), ("bayer_rggb8", 0)])
def test_every_push_mode(gpu_ctx, oracle, fmt, shift):
    """Host (dense and with pitch = w * bpp + 6), host batch, device copy (on_device 1), borrowed device (on_device 2) and
    device frames give the same bytes in all four levels of both cameras; a borrowed source is byte-identical after the push;
    after a borrowed push and a mskf_ctx_sync the caller overwrites its images, and the next frame's temporal track still sees
    the converted plane (== a stream that was pushed host images)."""
    w, h = 188, 120
    a, b = _pair(w, h, fmt, 0, shift)
    a2, b2 = np.roll(a, 1, axis=1), np.roll(b, 1, axis=1)
    ca, cb = PR.convert(a, fmt, shift), PR.convert(b, fmt, shift)

    ref = _stream(gpu_ctx, oracle, w, h, fmt, shift)
    ref.push_stereo(a, b)
    want = _levels(ref)
    assert np.array_equal(want[0], ca) and np.array_equal(want[4], cb)
    m = ref.cell_maxima()
    top = m[m["score"] > 0][:40]
    pts = np.stack([top["x"], top["y"]], axis=1)
    assert len(pts) >= 8

    # pitched host
    s = _stream(gpu_ctx, oracle, w, h, fmt, shift)
    pa, pb = PR.raw_bytes(a, fmt, 6, fill=9), PR.raw_bytes(b, fmt, 6, fill=250)
    assert pa.shape == (h, w * PR.BPP[fmt] + 6)
    s.push_stereo(pa, pb, pitch=pa.shape[1])
    _same(_levels(s), want)
    s.close()

    # host batch
    s = _stream(gpu_ctx, oracle, w, h, fmt, shift)
    gpu_ctx.push_stereo_batch([s], [a], [b])
    _same(_levels(s), want)
    assert s.cell_maxima().tobytes() == m.tobytes()
    s.close()

    # device copy and borrowed device, sources between canaries (at odd addresses where the format allows it)
    oa, ob = (130, 144) if fmt == "gray16" else (131, 145)
    for on_device in (1, 2):
        s = _stream(gpu_ctx, oracle, w, h, fmt, shift)
        (ha, da), (hb, db) = _canary_buffer(PR.raw_bytes(a, fmt), oa), _canary_buffer(PR.raw_bytes(b, fmt), ob)
        gpu_ctx.push_stereo_batch([s], [da.data_ptr() + oa], [db.data_ptr() + ob], on_device=on_device)
        _same(_levels(s), want)
        assert np.array_equal(da.read(), ha) and np.array_equal(db.read(), hb)
        if on_device == 2:
            gpu_ctx.sync()
            da.zero(); db.zero()
            for x in (s, ref):
                x.swap()
            s.push_stereo(a2, b2)
            ref.push_stereo(a2, b2)
            _same(_levels(s), _levels(ref))
            assert np.array_equal(s.get_level(0, 0), ca)
            t_s, t_ref = s.track(pts, do_temporal=1), ref.track(pts, do_temporal=1)
            _same([t_s[k] for k in sorted(t_s)], [t_ref[k] for k in sorted(t_ref)])
        s.close()
    ref.close()

    # device frames (mskf_fe_frame_batch_begin goes through the same push): three frames of borrowed device images against
    # a stream that is pushed the same frames from the host
    s, ref = _stream(gpu_ctx, oracle, w, h, fmt, shift), _stream(gpu_ctx, oracle, w, h, fmt, shift)
    s.set_grid()
    for k in range(3):
        fa, fb = np.roll(a, k, axis=1), np.roll(b, k, axis=1)
        (ha, da), (hb, db) = _canary_buffer(PR.raw_bytes(fa, fmt), oa), _canary_buffer(PR.raw_bytes(fb, fmt), ob)
        gpu_ctx.frame_batch_begin([s], [(da.data_ptr() + oa, db.data_ptr() + ob)], [{}], on_device=2)
        gpu_ctx.frame_batch_end()
        ref.push_stereo(fa, fb)
        # (the frame has rotated the pyramids: its cam0 is now the previous image)
        _same(_levels(s, roles=(0, 2)), _levels(ref))
        assert np.array_equal(s.get_level(0, 0), PR.convert(fa, fmt, shift))
        assert np.array_equal(da.read(), ha) and np.array_equal(db.read(), hb)
        ref.swap()
    s.close(); ref.close()


def test_mixed_batch(gpu_ctx, oracle):
    """One push_stereo_batch over seven streams of three sizes and six formats, two of them GRAY8, one converting stream and
    one GRAY8 stream equalising: every stream equals its solo push, the converting ones the restatement, and the plain GRAY8
    stream holds the image it was pushed and the oracle's pyramid of it."""
    shapes = [(188, 120), (333, 251), (188, 120), (64, 72), (333, 251), (188, 120), (64, 72)]
    fmts = [("gray8", 0), ("gray16", 4), ("rgb8", 0), ("bayer_gbrg8", 0), ("gray8", 0), ("bgra8", 0), ("gray16", 8)]
    eqs = [None, None, ("clahe", (5, 4), 3.0), None, ("hist", (8, 8), 40.0), None, None]
    pairs = [_pair(w, h, f, k, sh) for k, ((w, h), (f, sh)) in enumerate(zip(shapes, fmts))]

    def make(i):
        (w, h), (f, sh) = shapes[i], fmts[i]
        s = _stream(gpu_ctx, oracle, w, h, None if f == "gray8" else f, sh)
        if eqs[i]:
            s.set_equalize(*eqs[i])
        return s
    ss = [make(i) for i in range(len(shapes))]
    gpu_ctx.push_stereo_batch(ss, [p[0] for p in pairs], [p[1] for p in pairs])
    got = [[s.cell_maxima()] + _levels(s) for s in ss]
    for i, (pair, g) in enumerate(zip(pairs, got)):
        f, sh = fmts[i]
        solo = make(i)
        solo.push_stereo(*pair)
        _same(g, [solo.cell_maxima()] + _levels(solo))
        solo.close()
        for cam in (0, 1):
            conv = PR.convert(pair[cam], f, sh)
            if eqs[i]:
                conv = ER.equalize(conv, ER_MODE[eqs[i][0]], eqs[i][1], eqs[i][2])
            assert np.array_equal(g[1 + 4 * cam], conv), (i, cam)
            if f == "gray8" and not eqs[i]:
                ref = oracle.build_pyramid(pair[cam])
                for l in range(4):
                    assert np.array_equal(g[1 + 4 * cam + l], ref[l]), (cam, l)
    for s in ss:
        s.close()


ER_MODE = {"hist": 1, "clahe": 2}


@pytest.mark.parametrize("fmt,shift", [("gray16", 4), ("rgb8", 0), ("bayer_bggr8", 0)])
def test_conversion_then_equalisation(gpu_ctx, oracle, fmt, shift):
    """With the equalisation on (global, and CLAHE 8 x 8 / clip 40) level 0 == equalize_reference(convert_reference(raw)): the
    equalisation runs on the converted plane, for host and for borrowed device images."""
    w, h = 188, 120
    a, b = _pair(w, h, fmt, 2, shift)
    for mode, tiles, clip in (("hist", (8, 8), 40.0), ("clahe", (8, 8), 40.0)):
        want = [ER.equalize(PR.convert(x, fmt, shift), ER_MODE[mode], tiles, clip) for x in (a, b)]
        s = _stream(gpu_ctx, oracle, w, h, fmt, shift)
        s.set_equalize(mode, tiles, clip)
        s.push_stereo(a, b)
        assert np.array_equal(s.get_level(1, 0), want[0]) and np.array_equal(s.get_level(2, 0), want[1]), mode
        host_levels = _levels(s)
        s.swap()
        da, db = _Dev(PR.raw_bytes(a, fmt)), _Dev(PR.raw_bytes(b, fmt))
        gpu_ctx.push_stereo_batch([s], [da.data_ptr()], [db.data_ptr()], on_device=2)
        _same(_levels(s), host_levels)
        assert np.array_equal(da.read(), da.host) and np.array_equal(db.read(), db.host)
        s.close()


def _status(call, *a, **kw):
    try:
        call(*a, **kw)
        return 0
    except capi.MskfError as e:
        return e.code


def test_setter_and_push_refusals(gpu_ctx, oracle):
    """Every bad argument of the setter is refused with MSKF_ERR_INVALID, its message checked, and changes nothing; the setter is
    refused while a track batch or a device frame of the context is pending; the getter returns what was set; a GRAY16 push
    with an odd pointer or pitch, or a pitch under w * bpp, leaves the stream as it was and the next good push works; setting
    gray8 again restores today's behaviour (the planes equal a fresh GRAY8 stream's)."""
    w, h = 188, 120
    L = gpu_ctx.L
    s = _stream(gpu_ctx, oracle, w, h)
    assert s.get_input_format() == (0, 0)
    s.set_input_format("gray16", 4)
    assert s.get_input_format() == (1, 4)
    for bad, msg in [((10, 0), b"unknown format"), ((-1, 0), b"unknown format"), ((1, 9), b"shift must be 0 .. 8"), ((1, -1), b"shift must be 0 .. 8"),
                     ((2, 4), b"MSKF_PIX_GRAY16 only"), ((0, 1), b"MSKF_PIX_GRAY16 only"), ((9, 8), b"MSKF_PIX_GRAY16 only"), ((2, 9), b"shift must be 0 .. 8")]:
        assert _status(s.set_input_format, *bad) == -1, bad
        assert msg in L.mskf_last_error(), (bad, L.mskf_last_error())
        assert s.get_input_format() == (1, 4)
    assert _status(s.set_input_format, "yuv422") == -1
    L.mskf_fe_set_input_format.argtypes = [C.c_void_p, C.c_void_p]
    assert L.mskf_fe_set_input_format(s.h, None) == -1 and L.mskf_fe_set_input_format(None, None) == -1
    for name, num in PR.FORMATS.items():
        s.set_input_format(name, 8 if name == "gray16" else 0)
        assert s.get_input_format() == (num, 8 if name == "gray16" else 0)
    s.set_input_format("gray16", 4)

    a, b = _pair(w, h, "gray16", 0, 4)
    s.push_stereo(a, b)
    ca = PR.convert(a, "gray16", 4)
    before = _levels(s)
    assert np.array_equal(before[0], ca)
    # a GRAY16 push that is not 2-byte aligned: device images at an odd address, host rows of an odd pitch; and rows too short
    da, db = _Dev(np.zeros(2 * w * h + 16, np.uint8)), _Dev(np.zeros(2 * w * h + 16, np.uint8))
    for on_device in (1, 2):
        assert _status(gpu_ctx.push_stereo_batch, [s], [da.data_ptr() + 1], [db.data_ptr()], on_device=on_device) == -1
        assert b"2-byte aligned" in L.mskf_last_error()
        assert _status(gpu_ctx.push_stereo_batch, [s], [da.data_ptr()], [db.data_ptr() + 3], on_device=on_device) == -1
    odd = np.zeros((h, 2 * w + 7), np.uint8)
    assert _status(s.push_stereo, odd, odd, pitch=2 * w + 7) == -1 and b"2-byte aligned" in L.mskf_last_error()
    short = np.zeros((h, 2 * w - 2), np.uint8)
    assert _status(s.push_stereo, short, short, pitch=2 * w - 2) == -1 and b"differs from the calibration" in L.mskf_last_error()
    _same(_levels(s), before)
    a2, b2 = _pair(w, h, "gray16", 1, 4)
    s.push_stereo(a2, b2)
    assert np.array_equal(s.get_level(1, 0), PR.convert(a2, "gray16", 4)) and np.array_equal(s.get_level(2, 0), PR.convert(b2, "gray16", 4))

    # pending track batch, pending device frame
    gpu_ctx.track_batch_begin([s], [dict(pts=np.array([[40.0, 40.0], [90.0, 60.0]]), do_temporal=0)])
    try:
        assert _status(s.set_input_format, "rgb8") == -1 and b"track batch" in L.mskf_last_error()
    finally:
        gpu_ctx.track_batch_end()
    assert s.get_input_format() == (1, 4)
    s.swap()
    s.set_grid()
    gpu_ctx.frame_batch_begin([s], [(a, b)], [{}])
    try:
        assert _status(s.set_input_format, "gray8") == -1 and b"device frame" in L.mskf_last_error()
    finally:
        gpu_ctx.frame_batch_end()
    assert s.get_input_format() == (1, 4)
    s.close()

    # back to gray8: the stream is a GRAY8 stream again (host, pitched host and borrowed device pushes)
    s, fresh = _stream(gpu_ctx, oracle, w, h, "rgba8"), _stream(gpu_ctx, oracle, w, h)
    s.push_stereo(*_pair(w, h, "rgba8"))
    s.swap()
    s.set_input_format("gray8")
    assert s.get_input_format() == (0, 0)
    g0, g1 = ER.structured_images(w, h, seed=4)["scene"], ER.structured_images(w, h, seed=4)["random"]
    got = []
    for x in (s, fresh):
        x.push_stereo(g0, g1)
        got.append([x.cell_maxima()] + _levels(x))          # (the maxima of a push are read before the context's next push)
    _same(*got)
    assert np.array_equal(s.get_level(1, 0), g0)
    d0, d1 = _Dev(g0), _Dev(g1)
    got = []
    for x in (s, fresh):
        x.swap()
        gpu_ctx.push_stereo_batch([x], [d0.data_ptr()], [d1.data_ptr()], on_device=2)
        got.append([x.cell_maxima()] + _levels(x))
    _same(*got)
    s.close(); fresh.close()


# ------------------------------------------------------------------------------------------ the whole system
# 40 frames: the filter publishes its first pose once it has seen 200 IMU samples (frame 20 of these streams), and a comparison of
# poses and covariances needs some
_SYS = dict(w=188, h=120, n_frames=40, seed=0x5EED00A0)


def _colour(a, k=0):
    """An RGB image with genuinely different channels from a grey frame: the frame, its negative at half contrast, and the
    frame moved three pixels to the right."""
    return np.stack([a, (160 - a // 2).astype(np.uint8), np.roll(a, 3, axis=1)], axis=-1)


def _run_steps(oracle, fmt, shift, frames_of, n_frames):
    """A Runner of one fed frame by frame in the reference harness's call order; frames_of(a, b) maps the rendered pair to what
    the Runner is given."""
    from msckf_stereo_c_amd import runner as R
    syn = oracle.Synth(seed=_SYS["seed"], width=_SYS["w"], height=_SYS["h"])
    run = R.Runner(syn.calib, default_fe_cfg(), default_ekf_cfg(), 1, 1)
    run.publish_covariance(True)
    if fmt is not None:
        run.set_input_format(fmt, shift)
    view = R.StreamView(run)
    j, msgs = 0, []
    for k in range(n_frames):
        t_img = syn.frame_time(k)
        while True:
            s = syn.imu(j)
            j += 1
            view.imu(s)
            if not (s.time_stamp <= t_img):
                break
        view.stereo(*frames_of(*syn.render(k)), t_img)
        view.backend()
        msgs.append(run.msg(0).copy())
    return run, msgs


def _same_run(a, i, b, j, min_poses=10):
    """Stream i of runner a == stream j of runner b, bit for bit."""
    for x, y in zip(a.dump(i)[:4], b.dump(j)[:4]):
        assert np.array_equal(x, y)
    assert len(a.dump(i)[0]) > 0
    pa, pb = a.poses(i), b.poses(j)
    assert len(pa) == len(pb) >= min_poses, (len(pa), len(pb))
    assert pa.tobytes() == pb.tobytes()
    assert a.odom_cov(i).tobytes() == b.odom_cov(j).tobytes()
    assert np.array_equal(a.cov(i), b.cov(j))
    assert a.num_updates(i) == b.num_updates(j)


def test_runner_gray16_and_rgb8_match_gray8_runners(oracle):
    """(a) gray16 frames (g << 4) | low-bit noise with shift 4: messages, poses and covariances bitwise equal to a GRAY8 Runner on
    g (which the system tests tie to the oracle).  (b) rgb8 frames with genuinely different channels: bitwise equal to a GRAY8
    Runner fed the restatement's output."""
    n = _SYS["n_frames"]
    rng = np.random.default_rng(11)

    def noisy16(a, b):
        return tuple((x.astype(np.uint16) << 4) | rng.integers(0, 16, x.shape).astype(np.uint16) for x in (a, b))
    plain, m_plain = _run_steps(oracle, None, 0, lambda a, b: (a, b), n)
    g16, m_g16 = _run_steps(oracle, "gray16", 4, noisy16, n)
    assert len(m_plain) == len(m_g16) and all(x.tobytes() == y.tobytes() for x, y in zip(m_plain, m_g16))
    assert sum(len(x) for x in m_plain) > 0
    _same_run(g16, 0, plain, 0)
    print("gray16 runner: %d poses, %d updates, %d features in the last message" % (len(g16.poses(0)), g16.num_updates(0), len(m_g16[-1])))
    g16.close(); plain.close()

    rgb, m_rgb = _run_steps(oracle, "rgb8", 0, lambda a, b: (_colour(a), _colour(b)), n)
    conv, m_conv = _run_steps(oracle, None, 0, lambda a, b: (PR.convert(_colour(a), "rgb8"), PR.convert(_colour(b), "rgb8")), n)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(m_rgb, m_conv)) and sum(len(x) for x in m_rgb) > 0
    _same_run(rgb, 0, conv, 0)
    frame = oracle.Synth(seed=_SYS["seed"], width=_SYS["w"], height=_SYS["h"]).render(0)[0]
    assert not np.array_equal(PR.convert(_colour(frame), "rgb8"), frame)          # (the colour frames are not the grey ones in disguise)
    rgb.close(); conv.close()


def test_runner_device_resident_rgb8_sequence_pipelined_equals_lockstep(oracle):
    """(c) A device-resident rgb8 sequence (set_sequence with frame_bytes = 3 w h, borrowed device frames): a pipelined run ==
    the lockstep run == a GRAY8 Runner over the host sequence of the converted frames."""
    from msckf_stereo_c_amd import runner as R
    from msckf_stereo_c_amd.runner import IMU_SAMPLE
    w, h, n_frames = _SYS["w"], _SYS["h"], _SYS["n_frames"]
    syn = oracle.Synth(seed=_SYS["seed"] + 1, width=w, height=h)
    n_keys = syn.n_static + syn.n_loop
    rgb = np.zeros((2, n_keys, h, w, 3), np.uint8)
    grey = np.zeros((2, n_keys, h, w), np.uint8)
    for k in range(min(n_keys, n_frames + 1)):
        for c, x in enumerate(syn.render(k)):
            rgb[c, k] = _colour(x)
            grey[c, k] = PR.convert(rgb[c, k], "rgb8")
    imu = np.zeros((n_frames + 3) * 10 + 20, IMU_SAMPLE)
    for j in range(len(imu)):
        s = syn.imu(j)
        imu[j] = (s.time_stamp, tuple(s.angular_velocity), tuple(s.linear_acceleration))
    dev = _Dev(rgb)
    fe, ekf = default_fe_cfg(), default_ekf_cfg()
    runs = []
    for fmt, pipelined in (("rgb8", False), ("rgb8", True), (None, False)):
        run = R.Runner(syn.calib, fe, ekf, 1, 1, host_threads=1)
        if fmt:
            run.set_input_format(fmt)
            fb = 3 * w * h
            run.set_sequence(0, dev.data_ptr(), dev.data_ptr() + n_keys * fb, 2, fb, syn.n_static, syn.n_loop, 1403715273262142976, 50000000, imu)
        else:
            fb = w * h
            run.set_sequence(0, grey.ctypes.data, grey.ctypes.data + n_keys * fb, 0, fb, syn.n_static, syn.n_loop, 1403715273262142976, 50000000, imu)
        run.run(0, n_frames, threaded=True, pipelined=pipelined)
        runs.append(run)
    _same_run(runs[1], 0, runs[0], 0)
    _same_run(runs[0], 0, runs[2], 0)
    assert np.array_equal(dev.read(), rgb)
    for r in runs:
        r.close()


def test_runner_set_input_format_refuses_bad_arguments(oracle):
    from msckf_stereo_c_amd import runner as R
    syn = oracle.Synth(seed=1, width=188, height=120)
    run = R.Runner(syn.calib, default_fe_cfg(), default_ekf_cfg(), 1, 2)
    for bad in [dict(fmt=10), dict(fmt="yuv422"), dict(fmt="gray16", shift=9), dict(fmt="rgb8", shift=4), dict(fmt="gray16", shift=-1), dict(fmt="gray16", shift=4, stream=2)]:
        with pytest.raises(capi.MskfError):
            run.set_input_format(**bad)
    run.set_input_format("gray16", 4, stream=1)
    a = syn.render(0)[0]
    with pytest.raises(ValueError):          # stream 1 takes uint16 images now
        run.step([a, a], [a, a], [0.0, 0.0])
    with pytest.raises(ValueError):          # ... of the calibration's size
        run.step([a, a.astype(np.uint16)[:, :-2]], [a, a.astype(np.uint16)[:, :-2]], [0.0, 0.0])
    run.close()


# ------------------------------------------------------------------------------------------ the headless app
def _write_pnm(path, img):
    """Binary PGM (8-bit, or 16-bit big-endian) / PPM of an (h, w) or (h, w, 3) array."""
    h, w = img.shape[:2]
    if img.ndim == 3:
        head, body = "P6\n%d %d\n255\n" % (w, h), np.ascontiguousarray(img, dtype=np.uint8).tobytes()
    elif img.dtype == np.uint16:
        head, body = "P5\n%d %d\n65535\n" % (w, h), img.astype(">u2").tobytes()
    else:
        head, body = "P5\n%d %d\n255\n" % (w, h), np.ascontiguousarray(img, dtype=np.uint8).tobytes()
    with open(path, "wb") as f:
        f.write(head.encode() + body)


def _write_png(path, img):
    """8-bit grey, 16-bit grey, RGB or RGBA PNG with Pillow, which the project's other app tests (test_gpu_app.py,
    test_gpu_equalize.py, test_gpu_odom_cov.py) already write their PNGs with."""
    from PIL import Image
    if img.dtype == np.uint16:
        Image.frombytes("I;16", (img.shape[1], img.shape[0]), img.astype("<u2").tobytes()).save(path)
    else:
        Image.fromarray(img).save(path)


def _write_mav0(mav0, syn, n_frames, frames_of, writers):
    """A synthetic EuRoC mav0: frames_of(rendered image) is what is stored, writers[c] = (extension, function) per camera."""
    for c in (0, 1):
        (mav0 / ("cam%d" % c) / "data").mkdir(parents=True)
    (mav0 / "imu0").mkdir()
    t0_ns, dt_ns = 1403715273262142976, 50000000
    rows = [[], []]
    for k in range(n_frames):
        for c, x in enumerate(syn.render(k)):
            name = "%d.%s" % (t0_ns + k * dt_ns, writers[c][0])
            writers[c][1](mav0 / ("cam%d" % c) / "data" / name, frames_of(x))
            rows[c].append("%d,%s\r" % (t0_ns + k * dt_ns, name))
    for c in (0, 1):
        (mav0 / ("cam%d" % c) / "data.csv").write_text("#timestamp [ns],filename\r\n" + "\n".join(rows[c]) + "\n")
    lines = ["#timestamp [ns],w_x,w_y,w_z,a_x,a_y,a_z"]
    for j in range((n_frames + 2) * 10):
        s = syn.imu(j)
        vals = list(s.angular_velocity) + list(s.linear_acceleration)
        lines.append("%d,%s" % (t0_ns + j * (dt_ns // 10), ",".join("%.9g" % v for v in vals)))
    (mav0 / "imu0" / "data.csv").write_text("\n".join(lines) + "\n")


def _run_app(tmp_path, tag, mav0, yaml_tail):
    import shutil
    from msckf_stereo_c_amd import build
    build.build_all()
    top = tmp_path / tag
    shutil.copytree(os.path.join(ROOT, "config"), top / "config")
    with open(top / "config" / "app_imgproc.yaml", "a") as f:
        f.write(yaml_tail)
    work = top / "build"
    work.mkdir()
    exe = os.path.join(ROOT, "msckf_stereo_c_amd", "_build", "run_euroc_single_thread")
    res = subprocess.run([exe, str(mav0)], cwd=work, capture_output=True, text=True, timeout=120)
    pose = work / "pose_out.txt"
    return res, (pose.read_text().splitlines() if pose.exists() else [])


_APP = dict(n_frames=40, w=752, h=480)


@pytest.mark.parametrize("fmt", ["gray16", "rgb8"])
def test_app_reads_raw_files_with_input_format(tmp_path, oracle, fmt):
    """The headless app with input_format / input_shift in its app_imgproc.yaml on a short synthetic mav0 of 16-bit files (cam0
    PGM, cam1 PNG) or colour files (cam0 PNG, cam1 PPM) writes, line by line, the pose_out.txt of a run with the default
    configuration on the 8-bit files of the converted images."""
    n = _APP["n_frames"]
    syn = oracle.Synth(seed=0x5EED0042, width=_APP["w"], height=_APP["h"], n_static=21, motion_scale=3.0)
    rng = np.random.default_rng(3)
    if fmt == "gray16":
        def raw_of(x):
            return (x.astype(np.uint16) << 2) | rng.integers(0, 4, x.shape).astype(np.uint16)       # 10-bit data
        tail, shift, writers = "\ninput_format: gray16\ninput_shift: 2\n", 2, [("pgm", _write_pnm), ("png", _write_png)]
    else:
        raw_of, tail, shift, writers = _colour, "\ninput_format: rgb8\n", 0, [("png", _write_png), ("ppm", _write_pnm)]
    _write_mav0(tmp_path / "raw" / "mav0", syn, n, raw_of, writers)
    rng = np.random.default_rng(3)           # (the same noise again)
    _write_mav0(tmp_path / "conv" / "mav0", syn, n, lambda x: PR.convert(raw_of(x), fmt, shift), [("pgm", _write_pnm), ("png", _write_png)])
    res, got = _run_app(tmp_path, "a", tmp_path / "raw" / "mav0", tail)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    res, want = _run_app(tmp_path, "b", tmp_path / "conv" / "mav0", "\n")
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    print("%s: %d pose lines" % (fmt, len(got)))
    assert len(got) == len(want) > 5
    assert got == want


def test_app_refuses_a_file_that_does_not_fit_the_format(tmp_path, oracle):
    """8-bit grey files with input_format: gray16, and with rgb8: an error message and a non-zero exit status, no guess; the same
    files as a Bayer mosaic are taken (a Bayer file is an 8-bit grey file); an unknown input_format name fails the start."""
    syn = oracle.Synth(seed=0x5EED0042, width=_APP["w"], height=_APP["h"], n_static=21, motion_scale=3.0)
    _write_mav0(tmp_path / "mav0", syn, 2, lambda x: x, [("pgm", _write_pnm), ("png", _write_png)])
    for k, (tail, ok, msg) in enumerate([("\ninput_format: gray16\ninput_shift: 4\n", False, "takes 16-bit grey files"), ("\ninput_format: rgb8\n", False, "takes 8-bit RGB files"),
                                         ("\ninput_format: bayer_rggb8\n", True, ""), ("\ninput_format: yuv422\n", False, "input_format must be")]):
        res, _ = _run_app(tmp_path, "r%d" % k, tmp_path / "mav0", tail)
        assert (res.returncode == 0) == ok, (tail, res.returncode, res.stderr[-1000:])
        assert msg in res.stderr, (tail, res.stderr[-1000:])
