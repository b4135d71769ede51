"""Opt-in equalisation of pushed images on the device (mskf_fe_set_equalize; k_eq_hist / k_eq_lut / k_eq_apply) against the
numpy restatement of the contract (tests/equalize_reference.py), bit for bit."""
import ctypes as C

import numpy as np
import pytest

import equalize_reference as ER
from msckf_stereo_c_amd import capi
from msckf_stereo_c_amd.ctypes_types import default_ekf_cfg, default_fe_cfg

pytestmark = pytest.mark.gpu

HIST, CLAHE = 1, 2
# (mode, tiles, clip_limit): both modes, tiles 1 x 1, 5 x 4 and 8 x 8
CONFIGS = [(HIST, (8, 8), 40.0), (CLAHE, (1, 1), 40.0), (CLAHE, (5, 4), 3.0), (CLAHE, (8, 8), 40.0), (CLAHE, (8, 8), 0.0)]
KINDS = ["scene", "lowcontrast", "random", "step", "checker", "flat", "saturated", "ramp"]


def _stream(ctx, oracle, w, h):
    return capi.Stream(ctx, oracle.euroc_calib(w, h), default_fe_cfg(), default_ekf_cfg())


def _pair(w, h, k=0):
    """Two different images of the shared set (the kinds rotate with k)."""
    imgs = ER.structured_images(w, h, seed=k)
    return imgs[KINDS[k % len(KINDS)]], imgs[KINDS[(k + 1) % len(KINDS)]]


def _levels(s):
    return [s.get_level(role, l) for role in (1, 2) for l in range(4)]


def _same(a, b):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), (i, int((x != y).sum()) if x.shape == y.shape else None)


class _Dev:
    """A device buffer holding a copy of a host array, through the HIP runtime the product library itself is linked against
    (the test process holds that library only)."""

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


def _dev(arr):
    return _Dev(arr)


class EqJob(C.Structure):
    """EqJob of csrc/hip/fe_equalize.h: one image of the equalisation kernels.  tests/cpp/fe_equalize_test.cpp reports the header's
    own size and field offsets (eq_job_layout), which test_eq_job_layout_matches_the_header compares with this mirror."""
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("part", C.c_void_p), ("lut", C.c_void_p),
                ("w", C.c_int32), ("h", C.c_int32), ("mode", C.c_int32),
                ("tiles_x", C.c_int32), ("tiles_y", C.c_int32), ("tw", C.c_int32), ("th", C.c_int32), ("clip", C.c_int32),
                ("strip_rows", C.c_int32), ("n_strips", C.c_int32), ("_pad", C.c_int32)]


def _launch_equalize(ctx, jobs_dev, n_jobs, max_units, any_global, max_regions, splits):
    """fe_launch_equalize (what an equalising push enqueues: k_eq_hist, k_eq_lut, k_eq_apply) on the context's HIP stream."""
    f = ctx.L.fe_launch_equalize
    f.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    f.restype = None
    f(jobs_dev, n_jobs, max_units, any_global, max_regions, splits, ctx.hip_stream())


def test_eq_job_layout_matches_the_header(tmp_path):
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    so = str(tmp_path / "libfe_equalize_test.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-I", root, "-o", so,
                           os.path.join(root, "tests", "cpp", "fe_equalize_test.cpp")])
    out = (C.c_int * 16)()
    n = C.CDLL(so).eq_job_layout(out, 16)
    assert n == len(EqJob._fields_) + 1
    assert list(out[:n]) == [C.sizeof(EqJob)] + [getattr(EqJob, name).offset for name, _ in EqJob._fields_]


def _launch_direct(ctx, jobs):
    """The three kernels over bare images, as an equalising push enqueues them (fe_launch_equalize), for sizes no stream can
    have.  jobs: dicts(img, mode, tiles, clip_limit, offset, inplace, strip_rows).  The tile size and the clip come from the
    restatement, not from the header.  Every source sits `offset` bytes into a buffer with 64 canary bytes either side;
    the strips of the global mode and the row shares of the apply kernel are chosen odd on purpose (any split is valid).
    Returns the outputs and checks the canaries and (out of place) the sources."""
    recs, keep = (EqJob * len(jobs))(), []
    max_units, any_global, max_regions = 1, 0, 1
    for r, j in zip(recs, jobs):
        img = np.ascontiguousarray(j["img"], dtype=np.uint8)
        h, w = img.shape
        off = 64 + j.get("offset", 0)
        host = np.full(off + w * h + 64 + 16, 0xA5, np.uint8)
        host[off:off + w * h] = img.reshape(-1)
        buf = _dev(host)
        inplace = j.get("inplace", False) and off % 16 == 0
        dst = None if inplace else _dev(np.full(w * h + 32, 0x5A, np.uint8))
        r.src, r.dst = buf.data_ptr() + off, buf.data_ptr() + off if inplace else dst.data_ptr()
        r.w, r.h, r.mode = w, h, j["mode"]
        tx, ty = j["tiles"]
        r.tiles_x, r.tiles_y = tx, ty
        if j["mode"] == CLAHE:
            r.tw, r.th = ER.tile_geometry(w, h, tx, ty)
            r.clip = ER.clip_of(j["clip_limit"], r.tw * r.th) or 0
            r.clip = min(r.clip, r.tw * r.th)
            lut = _dev(np.zeros(256 * tx * ty, np.uint8))
            part = None
            max_units, max_regions = max(max_units, tx * ty), max(max_regions, (tx + 1) * (ty + 1))
        else:
            r.strip_rows = j.get("strip_rows", 7)
            r.n_strips = (h + r.strip_rows - 1) // r.strip_rows
            lut = _dev(np.zeros(256, np.uint8))
            part = _dev(np.full(256 * r.n_strips, -1, np.int32))
            r.part = part.data_ptr()
            max_units, any_global = max(max_units, r.n_strips), 1
        r.lut = lut.data_ptr()
        keep.append((buf, dst, lut, part, host, off, inplace, w, h))
    recs_dev = _dev(np.frombuffer(bytes(recs), np.uint8).copy())
    _launch_equalize(ctx, recs_dev.data_ptr(), len(jobs), max_units, any_global, max_regions, 3)
    ctx.sync()
    outs = []
    for buf, dst, lut, part, host, off, inplace, w, h in keep:
        after = buf.read()
        if inplace:
            outs.append(after[off:off + w * h].reshape(h, w).copy())
            after[off:off + w * h] = host[off:off + w * h]
        else:
            d = dst.read()
            outs.append(d[:w * h].reshape(h, w).copy())
            assert (d[w * h:] == 0x5A).all()
        assert np.array_equal(after, host)          # canaries, and a source that is not the destination, untouched
    return outs


SIZES = [(16, 16), (40, 24), (67, 45), (188, 120), (333, 251), (64, 1024), (1024, 64), (752, 480)]       # w, h


@pytest.mark.parametrize("w,h", SIZES)
def test_equalized_level0_bit_exact(gpu_ctx, oracle, w, h):
    """Level 0 of both cameras after an equalising push == the restatement, for both modes and tiles 1 x 1, 5 x 4, 8 x 8 (a
    size-and-tile pair the setter refuses is skipped: more tiles than pixels in a dimension); levels 1 .. 3 and the cell maxima
    == those of a second stream that was pushed the CPU-equalised images with the feature off.
    mskf_stream_create refuses images under 64 pixels in a dimension, so 16 x 16, 40 x 24 (tiles narrower than a 16-byte
    access) and 67 x 45 cannot be pushed: they run the same three kernels over bare images through fe_launch_equalize, in one
    batch, sources at unaligned addresses, out of place and in place."""
    configs = [c for c in CONFIGS if c[1][0] <= w and c[1][1] <= h]
    if w < 64 or h < 64:
        jobs, want = [], []
        for k, (mode, tiles, clip) in enumerate(configs):
            for n, img in enumerate(_pair(w, h, k)):
                for offset, inplace in ((0, True), (5, False), (16 + 11 * n, False)):
                    jobs.append(dict(img=img, mode=mode, tiles=tiles, clip_limit=clip, offset=offset, inplace=inplace, strip_rows=1 + 3 * n))
                    want.append(ER.equalize(img, mode, tiles, clip))
        _same(_launch_direct(gpu_ctx, jobs), want)
        return
    s, plain = _stream(gpu_ctx, oracle, w, h), _stream(gpu_ctx, oracle, w, h)
    for k, (mode, tiles, clip) in enumerate(configs if (w, h) != (752, 480) else [configs[0], configs[3]]):
        a, b = _pair(w, h, k)
        s.set_equalize(mode, tiles, clip)
        s.push_stereo(a, b)
        ea, eb = ER.equalize(a, mode, tiles, clip), ER.equalize(b, mode, tiles, clip)
        assert np.array_equal(s.get_level(1, 0), ea), (mode, tiles, clip, "cam0")
        assert np.array_equal(s.get_level(2, 0), eb), (mode, tiles, clip, "cam1")
        maxima = s.cell_maxima()
        got = _levels(s)
        plain.push_stereo(ea, eb)
        assert maxima.tobytes() == plain.cell_maxima().tobytes()
        _same(got, _levels(plain))
        s.swap(); plain.swap()
    s.close(); plain.close()


def test_bare_images_at_stream_sizes_and_splits(gpu_ctx):
    """The kernels' own edges at a size a stream can have, through fe_launch_equalize: a source whose first and last 16-byte
    chunk reach past the plane (offsets 1 .. 15), strips of one row and of more rows than the image, a ragged size."""
    w, h = 203, 77
    jobs, want = [], []
    for k, (mode, tiles, clip) in enumerate(CONFIGS):
        img = _pair(w, h, k)[0]
        for offset, strip_rows in ((1, 1), (15, 100), (8, 13)):
            jobs.append(dict(img=img, mode=mode, tiles=tiles, clip_limit=clip, offset=offset, strip_rows=strip_rows))
            want.append(ER.equalize(img, mode, tiles, clip))
    _same(_launch_direct(gpu_ctx, jobs), want)


def _canary_buffer(img, offset):
    host = np.full(256 + img.size + 256, 0xC3, np.uint8)
    host[offset:offset + img.size] = img.reshape(-1)
    return host, _dev(host)


@pytest.mark.parametrize("mode,tiles,clip", [(HIST, (8, 8), 40.0), (CLAHE, (8, 8), 40.0), (CLAHE, (5, 4), 3.0)])
def test_equalize_every_push_mode(gpu_ctx, oracle, mode, tiles, clip):
    """Host, pitched host, device copy (on_device 1), borrowed device (on_device 2) and a device frame give the same bytes in
    all four levels of both cameras; a borrowed source (at an unaligned address, canaries around it) is byte-identical after
    the push; after a borrowed push the caller overwrites its images, and the next frame's temporal track still sees the
    equalised plane (== a stream that was pushed host images)."""
    w, h = 188, 120
    a, b = _pair(w, h, 0)
    a2, b2 = np.roll(a, 1, axis=1), np.roll(b, 1, axis=1)
    ea, eb = ER.equalize(a, mode, tiles, clip), ER.equalize(b, mode, tiles, clip)

    ref = _stream(gpu_ctx, oracle, w, h)
    ref.set_equalize(mode, tiles, clip)
    ref.push_stereo(a, b)
    want = _levels(ref)
    assert np.array_equal(want[0], ea) and np.array_equal(want[4], eb)
    m = ref.cell_maxima()
    top = m[m["score"] > 0][:40]
    pts = np.stack([top["x"], top["y"]], axis=1)
    assert len(pts) >= 8

    # pitched host
    s = _stream(gpu_ctx, oracle, w, h)
    s.set_equalize(mode, tiles, clip)
    pa, pb = np.full((h, 200), 9, np.uint8), np.full((h, 200), 250, np.uint8)
    pa[:, :w], pb[:, :w] = a, b
    s.push_stereo(pa, pb, pitch=200)
    _same(_levels(s), want)
    s.close()

    # device copy and borrowed device, sources at unaligned addresses between canaries
    for on_device in (1, 2):
        s = _stream(gpu_ctx, oracle, w, h)
        s.set_equalize(mode, tiles, clip)
        (ha, da), (hb, db) = _canary_buffer(a, 131), _canary_buffer(b, 144)
        gpu_ctx.push_stereo_batch([s], [da.data_ptr() + 131], [db.data_ptr() + 144], on_device=on_device)
        _same(_levels(s), want)
        assert np.array_equal(da.read(), ha) and np.array_equal(db.read(), hb)
        if on_device == 2:
            # the caller reuses its buffers at once; the next frame tracks from the stream's own equalised plane
            da.zero(); db.zero()
            for x in (s, ref):
                x.swap()
            s.push_stereo(a2, b2)
            ref.push_stereo(a2, b2)
            _same(_levels(s), _levels(ref))
            assert np.array_equal(s.get_level(0, 0), ea)
            t_s, t_ref = s.track(pts, do_temporal=1), ref.track(pts, do_temporal=1)
            _same([t_s[k] for k in sorted(t_s)], [t_ref[k] for k in sorted(t_ref)])
        s.close()
    ref.close()

    # a device frame (mskf_fe_frame_batch_begin goes through the same push): borrowed device images
    s = _stream(gpu_ctx, oracle, w, h)
    s.set_equalize(mode, tiles, clip)
    s.set_grid()
    (ha, da), (hb, db) = _canary_buffer(a, 131), _canary_buffer(b, 144)
    gpu_ctx.frame_batch_begin([s], [(da.data_ptr() + 131, db.data_ptr() + 144)], [{}], on_device=2)
    gpu_ctx.frame_batch_end()
    # (the frame has rotated the pyramids: its cam0 is now the previous image)
    _same([s.get_level(0, l) for l in range(4)] + [s.get_level(2, l) for l in range(4)], want)
    assert np.array_equal(da.read(), ha) and np.array_equal(db.read(), hb)
    s.close()


def test_equalize_mixed_batch(gpu_ctx, oracle):
    """One push_stereo_batch over five streams of three sizes with modes 0 / 1 / 2 / 2 / 0 and different tiles: every stream
    equals its solo push, and the mode-0 streams hold the plain image and the oracle's pyramid of it."""
    shapes = [(188, 120), (333, 251), (188, 120), (64, 72), (333, 251)]
    cfgs = [(0, (8, 8), 40.0), (HIST, (8, 8), 40.0), (CLAHE, (8, 8), 40.0), (CLAHE, (5, 4), 3.0), (0, (8, 8), 40.0)]
    pairs = [_pair(w, h, k) for k, (w, h) in enumerate(shapes)]
    ss = []
    for (w, h), cfg in zip(shapes, cfgs):
        s = _stream(gpu_ctx, oracle, w, h)
        if cfg[0]:
            s.set_equalize(*cfg)
        assert s.get_equalize() == (cfg[0], cfg[1], cfg[2])
        ss.append(s)
    gpu_ctx.push_stereo_batch(ss, [p[0] for p in pairs], [p[1] for p in pairs])
    got = [[s.cell_maxima()] + _levels(s) for s in ss]
    for (w, h), cfg, pair, g in zip(shapes, cfgs, pairs, got):
        solo = _stream(gpu_ctx, oracle, w, h)
        solo.set_equalize(*cfg)
        solo.push_stereo(*pair)
        _same(g, [solo.cell_maxima()] + _levels(solo))
        solo.close()
        for cam in (0, 1):
            assert np.array_equal(g[1 + 4 * cam], ER.equalize(pair[cam], *cfg))
            if cfg[0] == 0:
                ref = oracle.build_pyramid(pair[cam])
                for l in range(4):
                    assert np.array_equal(g[1 + 4 * cam + l], ref[l]), (cam, l)
    for s in ss:
        s.close()


def _status(call, *a, **kw):
    try:
        call(*a, **kw)
        return 0
    except capi.MskfError as e:
        return e.code


def test_equalize_setter_refusals(gpu_ctx, oracle):
    """Every bad argument is refused with MSKF_ERR_INVALID and changes nothing; the setter is refused while a track batch or
    a device frame of the context is pending, and the message names the batch; the getter round-trips; a mode switched between
    pushes takes effect with the next push only."""
    w, h = 188, 120
    a, b = _pair(w, h, 0)
    L = gpu_ctx.L
    s = _stream(gpu_ctx, oracle, w, h)
    assert s.get_equalize()[0] == 0
    s.set_equalize("clahe", (5, 4), 3.0)
    assert s.get_equalize() == (2, (5, 4), 3.0)
    for bad in [(3, (8, 8), 40.0), (-1, (8, 8), 40.0), (2, (0, 8), 40.0), (2, (8, 0), 40.0), (2, (-2, 8), 40.0), (2, (w + 1, 8), 40.0), (2, (8, h + 1), 40.0),
                (2, (8, 8), -1.0), (2, (8, 8), float("nan")), (2, (8, 8), float("inf")), (1, (0, 0), 40.0), (1, (8, 8), -0.5)]:
        assert _status(s.set_equalize, *bad) == -1, bad
        assert len(L.mskf_last_error()) > 0
        assert s.get_equalize() == (2, (5, 4), 3.0)
    L.mskf_fe_set_equalize.argtypes = [C.c_void_p, C.c_void_p]
    assert L.mskf_fe_set_equalize(s.h, None) == -1 and L.mskf_fe_set_equalize(None, None) == -1
    assert _status(s.set_equalize, 2, (w, h), 40.0) == 0            # as many tiles as pixels is the limit
    s.set_equalize("clahe", (5, 4), 3.0)

    s.push_stereo(a, b)
    e2 = ER.equalize(a, 2, (5, 4), 3.0)
    assert np.array_equal(s.get_level(1, 0), e2)
    # pending track batch
    gpu_ctx.track_batch_begin([s], [dict(pts=np.array([[40.0, 40.0], [90.0, 60.0]]), do_temporal=0)])
    try:
        assert _status(s.set_equalize, 1) == -1 and b"track batch" in L.mskf_last_error()
    finally:
        gpu_ctx.track_batch_end()
    assert s.get_equalize() == (2, (5, 4), 3.0)
    # a mode switched between pushes: the pushed plane stays, the next push has the new mode
    s.set_equalize("hist")
    assert s.get_equalize()[0] == 1
    assert np.array_equal(s.get_level(1, 0), e2)
    s.swap()
    s.push_stereo(a, b)
    assert np.array_equal(s.get_level(1, 0), ER.equalize(a, 1)) and np.array_equal(s.get_level(0, 0), e2)
    # pending device frame
    s.swap()
    s.set_grid()
    gpu_ctx.frame_batch_begin([s], [(a, b)], [{}])
    try:
        assert _status(s.set_equalize, 0) == -1 and b"device frame" in L.mskf_last_error()
    finally:
        gpu_ctx.frame_batch_end()
    assert s.get_equalize()[0] == 1
    s.set_equalize("off")
    s.push_stereo(a, b)
    assert np.array_equal(s.get_level(1, 0), a)
    s.close()


# ------------------------------------------------------------------------------------------ the whole system
# Low-contrast frames: v' = 96 + v // 24, an integer rule.  Chosen on the CPU with the oracle over 40 frames of the 188 x 120
# stream below: the mean number of published features is 14.0 on the raw low-contrast frames and 62.25 on their CLAHE
# (8 x 8, clip 40).  The milder v' = 96 + v // 8 does not separate the two (62.9 raw, 65.4 equalised: the synthetic texture
# keeps its corners above the detector threshold at an eighth of the contrast); from // 32 on the raw run publishes nothing.
_SYS = dict(w=188, h=120, n_frames=40, seed=0x5EED0090, tiles=(8, 8), clip=40.0)


def _low(v):
    return (96 + v // 24).astype(np.uint8)


class _LowContrast:
    """A synthetic stream whose rendered frames are reduced in contrast (everything else is the generator's)."""

    def __init__(self, syn):
        self._syn = syn

    def __getattr__(self, name):
        return getattr(self._syn, name)

    def render(self, k):
        a, b = self._syn.render(k)
        return _low(a), _low(b)


def _lockstep_equalized(oracle, syn, equalize, n_frames):
    """Oracle and a Runner of one in lockstep (as tests/test_gpu_system.py::_lockstep): the Runner gets the frames of `syn` and,
    with `equalize`, equalises them on the device; the oracle gets the restatement's output.  Compared every frame.
    Returns (oracle, runner, published features per frame)."""
    from msckf_stereo_c_amd import runner as R
    from test_gpu_system import compare_frame
    fe, ekf = default_fe_cfg(), default_ekf_cfg()
    osys = oracle.OracleSystem(syn.calib, fe, ekf)
    run = R.Runner(syn.calib, fe, ekf, 1, 1)
    if equalize:
        run.set_equalize("clahe", _SYS["tiles"], _SYS["clip"])
    view = R.StreamView(run)
    j, counts = 0, []
    for k in range(n_frames):
        t_img = syn.frame_time(k)
        while True:
            s = syn.imu(j)
            j += 1
            osys.imu(s)
            view.imu(s)
            if not (s.time_stamp <= t_img):
                break
        a, b = syn.render(k)
        view.stereo(a, b, t_img)
        if equalize:
            a, b = ER.clahe(a, *_SYS["tiles"], _SYS["clip"]), ER.clahe(b, *_SYS["tiles"], _SYS["clip"])
        osys.stereo(a, b, t_img)
        osys.backend()
        view.backend()
        compare_frame(k, osys, run)
        counts.append(len(osys.dump()[0]))
    return osys, run, counts


def _same_run(a, i, b, j):
    """Stream i of runner a == stream j of runner b, bit for bit."""
    for x, y in zip(a.dump(i)[:4], b.dump(j)[:4]):
        assert np.array_equal(x, y)
    pa, pb = a.poses(i), b.poses(j)
    assert len(pa) == len(pb) > 10
    assert np.array_equal(pa["t"], pb["t"]) and np.array_equal(pa["p"], pb["p"]) and np.array_equal(pa["q"], pb["q"])
    assert np.array_equal(a.cov(i), b.cov(j))
    assert a.num_updates(i) == b.num_updates(j)


def test_runner_equalized_matches_oracle_on_equalized_images(oracle):
    """A Runner of one with CLAHE on, fed low-contrast frames == the oracle fed the restatement's output of the same frames, per
    frame: ids, lifetimes and pixels bit for bit, poses within the suite's 1e-4 m; a Runner with the feature off, fed the raw
    low-contrast frames == the oracle on those.  The two oracle runs are the yardstick of usefulness: the equalised run
    publishes more features on average (62.25 against 14.0, measured with the oracle on the CPU).  The same equalised stream
    through run(): pipelined == lockstep == the frame-by-frame run; and a batch of three streams with the feature on for one
    of them == three solo runs."""
    from msckf_stereo_c_amd import runner as R
    from test_gpu_system import _attach_sequences, compare_msgs, compare_poses
    w, h, n_frames = _SYS["w"], _SYS["h"], _SYS["n_frames"]
    syn = _LowContrast(oracle.Synth(seed=_SYS["seed"], width=w, height=h))
    o_eq, r_eq, c_eq = _lockstep_equalized(oracle, syn, True, n_frames)
    compare_msgs(o_eq, r_eq)
    compare_poses(o_eq, r_eq)
    o_raw, r_raw, c_raw = _lockstep_equalized(oracle, syn, False, n_frames)
    compare_msgs(o_raw, r_raw)
    compare_poses(o_raw, r_raw)
    print("mean published features: equalised %.2f, raw %.2f" % (np.mean(c_eq), np.mean(c_raw)))
    assert np.mean(c_eq) > np.mean(c_raw)
    r_raw.close()

    fe, ekf = default_fe_cfg(), default_ekf_cfg()
    keep = []
    for pipelined in (False, True):
        run = R.Runner(syn.calib, fe, ekf, 1, 1, host_threads=1)
        run.set_equalize("clahe", _SYS["tiles"], _SYS["clip"])
        _attach_sequences(oracle, run, [syn], n_frames, keep)
        run.run(0, n_frames, threaded=True, pipelined=pipelined)
        _same_run(run, 0, r_eq, 0)
        run.close()

    # three streams in one batch, the feature on for the middle one only
    syns = [_LowContrast(oracle.Synth(seed=_SYS["seed"] + i, width=w, height=h)) for i in range(3)]
    batch = R.Runner(syns[0].calib, fe, ekf, 1, 3, host_threads=1)
    batch.set_equalize("clahe", _SYS["tiles"], _SYS["clip"], stream=1)
    _attach_sequences(oracle, batch, syns, n_frames, keep)
    batch.run(0, n_frames, threaded=True, pipelined=False)
    for i in range(3):
        solo = R.Runner(syns[i].calib, fe, ekf, 1, 1, host_threads=1)
        if i == 1:
            solo.set_equalize("clahe", _SYS["tiles"], _SYS["clip"])
        _attach_sequences(oracle, solo, [syns[i]], n_frames, keep)
        solo.run(0, n_frames, threaded=True, pipelined=False)
        _same_run(batch, i, solo, 0)
        solo.close()
    assert len(batch.dump(1)[0]) > len(batch.dump(0)[0])          # (the equalised stream of the batch is the one that keeps its features)
    batch.close()
    r_eq.close()


def test_runner_set_equalize_refuses_bad_arguments(oracle):
    from msckf_stereo_c_amd import runner as R
    syn = oracle.Synth(seed=1, width=188, height=120)
    run = R.Runner(syn.calib, default_fe_cfg(), default_ekf_cfg(), 1, 2)
    for bad in [dict(mode=5), dict(mode="clahe", tiles=(0, 8)), dict(mode="clahe", clip_limit=-1.0), dict(mode="hist", stream=2)]:
        with pytest.raises(capi.MskfError):
            run.set_equalize(**bad)
    run.set_equalize("hist", stream=1)
    run.close()


def test_app_reads_equalize_keys(tmp_path, oracle):
    """The headless app with equalize / clahe_clip_limit / clahe_tiles_x / clahe_tiles_y in its app_imgproc.yaml writes the
    poses of a Runner of one with the same settings (pose_out.txt has six decimals) and logs its tracking counts, which are not
    those of a Runner with the feature off."""
    import os
    import shutil
    import subprocess
    from PIL import Image
    from msckf_stereo_c_amd import build
    from msckf_stereo_c_amd import runner as R
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    build.build_all()
    n_frames = 40
    syn = _LowContrast(oracle.Synth(seed=0x5EED0042, width=752, height=480, n_static=21, motion_scale=3.0))
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
    shutil.copytree(os.path.join(root, "config"), tmp_path / "config")
    with open(tmp_path / "config" / "app_imgproc.yaml", "a") as f:
        f.write("\nequalize: clahe\nclahe_clip_limit: 3.0\nclahe_tiles_x: 6\nclahe_tiles_y: 5\n")
    work = tmp_path / "build"
    work.mkdir()
    exe = os.path.join(root, "msckf_stereo_c_amd", "_build", "run_euroc_single_thread")
    res = subprocess.run([exe, str(mav0)], cwd=work, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    got = np.loadtxt(work / "pose_out.txt").reshape(-1, 8)

    # what the app parses (run_euroc_single_thread.cpp): stamps as seconds * 1e9 + nanoseconds in double, IMU values as float
    from msckf_stereo_c_amd.ctypes_types import ImuSample

    def stamp(ns):
        return (int(str(ns)[:-9]) * 1e9 + int(str(ns)[-9:])) * 1e-9
    imu = []
    for line in lines[1:]:
        f = line.split(",")
        v = [float(np.float32(x)) for x in f[1:7]]
        imu.append(ImuSample(stamp(int(f[0])), (C.c_double * 3)(*v[:3]), (C.c_double * 3)(*v[3:])))

    # ... and the configuration as the app reads it (the equalize keys are the app's own business: set below)
    from msckf_stereo_c_amd.ctypes_types import Calib, EkfCfg, FeCfg
    calib, fe, ekf = Calib(), FeCfg(), EkfCfg()
    assert R.lib().mskfh_load_configs(str(tmp_path / "config").encode(), C.byref(calib), C.byref(fe), C.byref(ekf)) == 0

    def runner_poses(equalize):
        run = R.Runner(calib, fe, ekf, 1, 1)
        if equalize:
            run.set_equalize("clahe", (6, 5), 3.0)
        view = R.StreamView(run)
        j = 0
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
        p, info = run.poses(0), run.dump(0)[4]
        run.close()
        return p, (info.before_tracking, info.after_tracking, info.after_matching, info.after_ransac)
    (want, info), (_, info_off) = runner_poses(True), runner_poses(False)
    # the last frame's tracking counts, as the app logs them: those of the equalising Runner, not those of the plain one
    last = (work / "debug_imageprocessor.txt").read_text().strip().splitlines()[-1]
    assert tuple(int(v) for v in last.split(":")[1].split(",")) == info != info_off
    assert len(got) == len(want) > 5
    assert np.abs(got[:, 0] - want["t"]).max() < 2e-6
    assert np.abs(got[:, 1:4] - want["p"]).max() <= 0.5e-6 + 1e-9 and np.abs(got[:, 4:8] - want["q"]).max() <= 0.5e-6 + 1e-9
