"""Opt-in deeper LK pyramids on the device (mskf_fe_set_lk_levels; k_pyr_down_deep, k_track4_deep, k_fb_points_deep) against the
numpy restatement of the L-level LK (tests/deep_lk_reference.py, pinned on the CPU by tests/test_deep_lk_reference.py; DESIGN.md §3,
"Deeper LK pyramids"), bit for bit: the extra pyramid levels of all three roles, their rotation, track calls at their count edges,
mixed batches, the forward-backward check, the device frame and the setter's refusals."""
import ctypes as C

import numpy as np
import pytest

import camera_models_cases as CMC
import deep_lk_reference as D
import fb_reference as FB
import frame_cases as F
import lk_cases as LC
import test_gpu_patch as GP
from msckf_stereo_c_amd import capi
from msckf_stereo_c_amd.ctypes_types import default_ekf_cfg, default_fe_cfg

from hip_runtime import Hip

pytestmark = pytest.mark.gpu

K_PYR, K_LK, K_PYR_DEEP = 0, 2, 12            # MSKF_K_PYR, MSKF_K_LK, MSKF_K_PYR_DEEP (the slot of MSKF_K_PT_GEOM, shared with the point gates)
NAMES = ("out0", "out1", "und0", "und1", "status")
COUNTS = (0, 1, 4, 5, 63)
_HIP_ERRORS = []                              # after a HIP error no test of this module launches anything


def _guarded(test):
    import functools

    @functools.wraps(test)
    def run(*a, **kw):
        assert not _HIP_ERRORS, "an earlier launch ended with a HIP error: %s" % _HIP_ERRORS
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


def _stream(ctx, oracle, w, h, levels=None, calib=None):
    s = capi.Stream(ctx, oracle.euroc_calib(w, h) if calib is None else calib, default_fe_cfg(), default_ekf_cfg())
    if levels is not None:
        s.set_lk_levels(levels)
    return s


def _status(call, *a, **kw):
    try:
        call(*a, **kw)
        return 0
    except capi.MskfError as e:
        return e.code


def _chain(img, levels):
    return D.pyramid(np.ascontiguousarray(img), levels)


def _images(w, h, seed):
    rng = np.random.default_rng(seed)
    return [np.ascontiguousarray((LC.smooth_canvas(w, h, seed + k)[:h, :w] // 2 + rng.integers(0, 128, (h, w))).astype(np.uint8)) for k in range(4)]


# ------------------------------------------------------------------------------------------ the extra pyramid levels
@pytest.mark.parametrize("w,h,levels,how", [(512, 480, 6, "host"), (517, 483, 6, "pitched"), (240, 240, 5, "device"), (512, 480, 6, "equalized")])
@_guarded
def test_pyramid_levels_and_swap(gpu_ctx, oracle, w, h, levels, how):
    """Levels 4 .. L - 1 of all three roles equal the pyr_down chain byte for byte (odd sides at every level, a 15 x 15 top level, a
    pitched host push, a device push, an equalised level 0), one launch of k_pyr_down_deep per push; after a second push and swap,
    prev0's deep levels are the first frame's."""
    a0, b0, a1, b1 = _images(w, h, 40 + w)
    s = _stream(gpu_ctx, oracle, w, h, levels)
    assert s.get_lk_levels() == levels
    if how == "equalized":
        s.set_equalize("clahe", (4, 4), 4.0)
    hip = Hip()
    keep = []                                  # (a padded host image is copied asynchronously: it has to outlive the push)

    def push(a, b):
        if how == "pitched":
            pitch = w + 27
            pa, pb = np.full((h, pitch), 77, np.uint8), np.full((h, pitch), 99, np.uint8)
            pa[:, :w], pb[:, :w] = a, b
            keep.extend([pa, pb])
            s.push_stereo(pa, pb, pitch=pitch)
        elif how == "device":
            da, db = hip.alloc(a.size, False), hip.alloc(b.size, False)
            hip.put(da, a)
            hip.put(db, b)
            gpu_ctx.push_stereo_batch([s], [da], [db], on_device=1)
        else:
            s.push_stereo(a, b)
    try:
        with GP._Timed(gpu_ctx) as t:
            push(a0, b0)
            gpu_ctx.sync()
        assert t.launches[K_PYR_DEEP] == 1 and t.launches[K_PYR] == 1
        first = {}
        for role, img in ((1, a0), (2, b0)):
            l0 = s.get_level(role, 0)
            assert np.array_equal(l0, img) == (how != "equalized")
            want = _chain(l0, levels)
            assert want[levels - 1].shape == tuple(reversed(D.level_sizes(w, h, levels)[levels - 1])) and min(want[levels - 1].shape) >= 15
            for l in range(levels):
                got = s.get_level(role, l)
                assert got.shape == want[l].shape and np.array_equal(got, want[l]), (role, l)
            first[role] = want
        assert _status(s.get_level, 1, levels) == -1
        s.swap()
        push(a1, b1)
        for l in range(levels):
            assert np.array_equal(s.get_level(0, l), first[1][l]), l          # prev0: the first frame's cam0, every level
            assert np.array_equal(s.get_level(1, l), _chain(s.get_level(1, 0), levels)[l]), l
            assert np.array_equal(s.get_level(2, l), _chain(s.get_level(2, 0), levels)[l]), l
        assert not np.array_equal(s.get_level(1, levels - 1), first[1][levels - 1])
    except BaseException as e:
        if not isinstance(e, AssertionError):
            _HIP_ERRORS.append(repr(e))
        raise
    finally:
        gpu_ctx.sync()
        s.close()
        hip.free()


# ------------------------------------------------------------------------------------------ track parity
TW, TH = 512, 480                 # level 5 is 16 x 15: every window of the top level overhangs the image
_REF = {}


def _scene(oracle, name):
    """(prev0, curr0, curr1, pts): the shifted smooth scene (36 px along x) or the border lattice, 63 points."""
    if ("scene", name) not in _REF:
        sx, sy = LC.stereo_shift(TW, TH, oracle)
        if name == "smooth":
            A, B, _ = D.scene(TW, TH, 36)
            pts = LC.lattice(TW, TH, pitch=41)
            pts = pts[pts[:, 0] < TW - 60][:63]
        else:
            c = [c for c in LC.cases("border", TW, TH, oracle) if c["name"] == "border_template"][0]
            A, B = c["A"], c["B"]
            pts = c["pts"][np.linspace(0, len(c["pts"]) - 1, 63).astype(int)]
        assert len(pts) == 63
        _REF[("scene", name)] = (A, B, LC.shifted_replicate(B, sx, sy), np.ascontiguousarray(pts, dtype=np.float32))
    return _REF[("scene", name)]


def _reference(oracle, name, levels, do_temporal):
    """The steps of frame_cases.track_reference / stereo_reference with the LK replaced by the restatement, per point (computed once)."""
    key = (name, levels, do_temporal)
    if key not in _REF:
        prev0, curr0, curr1, pts = _scene(oracle, name)
        calib, fe = oracle.euroc_calib(TW, TH), default_fe_cfg()
        DO = D.DeepOracle(oracle, levels)
        if do_temporal:
            r = F.track_reference(DO, calib, fe, prev0, curr0, curr1, pts)
        else:
            sub = F.stereo_reference(DO, calib, fe, curr0, curr1, pts)
            r = dict(ok=np.ones(len(pts), bool), **sub)
        _REF[key] = r
    return _REF[key]


def _assert_track(got, ref, n, tag):
    ok, inl = ref["ok"][:n], ref["inl"][:n]
    assert np.array_equal((got["status"] & 1).astype(bool), ok), tag
    assert np.array_equal(((got["status"] >> 1) & 1).astype(bool), inl & ok), tag
    for k, r in (("out0", "cam0"), ("out1", "cam1"), ("und0", "und0"), ("und1", "und1")):
        assert LC.same(got[k][ok], ref[r][:n][ok]), (tag, k)
        if k != "out0":
            assert (LC.bits(got[k][~ok]) == 0).all(), (tag, k)
    assert (got["status"][~ok] == 0).all(), tag


@pytest.mark.parametrize("name", ["smooth", "border"])
@pytest.mark.parametrize("levels", [5, 6])
@_guarded
def test_track_parity(gpu_ctx, oracle, name, levels):
    """Stream.track, temporal + stereo and stereo only, at 0, 1, 4, 5 and 63 points: positions, undistorted points and status bits
    are the restatement's; the deep instantiation is one launch."""
    prev0, curr0, curr1, pts = _scene(oracle, name)
    s = _stream(gpu_ctx, oracle, TW, TH, levels)
    s.push_stereo(prev0, prev0)
    s.swap()
    s.push_stereo(curr0, curr1)
    for do_temporal in (1, 0):
        ref = _reference(oracle, name, levels, do_temporal)
        assert ref["ok"].sum() >= 10 and ref["inl"].sum() >= 5, (name, levels, do_temporal)
        for n in COUNTS:
            with GP._Timed(gpu_ctx) as t:
                got = s.track(pts[:n], do_temporal)
            assert t.launches[K_LK] == (1 if n else 0)
            _assert_track(got, ref, n, (name, levels, do_temporal, n))
    # the depth matters on the shifted scene: four levels do not give these results
    if name == "smooth":
        r4, r = _reference(oracle, name, 4, 1), _reference(oracle, name, levels, 1)
        assert not np.array_equal(r4["ok"], r["ok"]) or not LC.same(r4["cam0"], r["cam0"])
    s.close()


@_guarded
def test_a_default_stream_loses_what_a_deep_stream_keeps(gpu_ctx, oracle):
    """The capture-range scene of the CPU test (640 x 512, 52 px): a default stream tracks what the oracle tracks (fewer than half of
    the points 8 px tracks), the same stream with six levels what the restatement keeps (at least 90 %).  Without the feature
    there is no setter: this test fails."""
    w, h, shift = 640, 512, 52
    A8, B8, pts = D.scene(w, h, 8)
    A, B, pts2 = D.scene(w, h, shift)
    assert np.array_equal(pts, pts2)
    sx, sy = LC.stereo_shift(w, h, oracle)
    base = D.tracked(*oracle.lk_track(A8, B8, pts, pts), pts, 8)
    kept = {}
    for levels in (None, 6):
        s = _stream(gpu_ctx, oracle, w, h, levels)
        assert s.get_lk_levels() == (levels or 4)
        s.push_stereo(A, A)
        s.swap()
        s.push_stereo(B, LC.shifted_replicate(B, sx, sy))
        got = s.track(pts, 1)
        ref_b, ref_st = D.lk_track(A, B, pts, pts, levels or 4)
        ok = ref_st.astype(bool) & LC.in_image(ref_b, w, h)
        assert np.array_equal((got["status"] & 1).astype(bool), ok) and LC.same(got["out0"][ok], ref_b[ok])
        kept[levels] = int((D.tracked(got["out0"], got["status"] & 1, pts, shift) & base).sum())
        s.close()
    n = int(base.sum())
    print("device, %d px: %d of %d at four levels, %d at six" % (shift, kept[None], n, kept[6]))
    assert n >= 30 and 2 * kept[None] < n and 10 * kept[6] >= 9 * n


# ------------------------------------------------------------------------------------------ mixed batches
@_guarded
def test_mixed_batch(gpu_ctx, oracle):
    """One track_batch with a four-level, a five-level and a six-level stream: the four-level stream's outputs equal those of the
    same call alone (k_track4), the others the restatement."""
    prev0, curr0, curr1, pts = _scene(oracle, "smooth")
    ss = [_stream(gpu_ctx, oracle, TW, TH, L) for L in (None, 5, 6)]
    for s in ss:
        s.push_stereo(prev0, prev0)
        s.swap()
    gpu_ctx.push_stereo_batch(ss, [curr0] * 3, [curr1] * 3)
    gpu_ctx.sync()
    counts = (63, 41, 5)
    with GP._Timed(gpu_ctx) as t:
        res = gpu_ctx.track_batch(ss, [dict(pts=pts[:n], do_temporal=1) for n in counts])
    assert t.launches[K_LK] == 1
    with GP._Timed(gpu_ctx) as t:
        alone = gpu_ctx.track_batch(ss[:1], [dict(pts=pts[:counts[0]], do_temporal=1)])[0]
    assert t.launches[K_LK] == 1
    for k in NAMES:
        assert alone[k].tobytes() == res[0][k].tobytes(), k
    _assert_track(res[0], _reference(oracle, "smooth", 4, 1), counts[0], "four levels")
    _assert_track(res[1], _reference(oracle, "smooth", 5, 1), counts[1], "five levels")
    _assert_track(res[2], _reference(oracle, "smooth", 6, 1), counts[2], "six levels")
    for s in ss:
        s.close()


@_guarded
def test_a_deep_stream_on_an_extended_camera_model(gpu_ctx, oracle):
    """A double-sphere stream that is also deep, in one batch with a plain one.  On a flat pair LK returns its guess at every
    depth, so the deep ds stream must give the bits of the same ds stream at four levels (k_track4_ext), domain refusals
    included: the extended geometry survives inside k_track4_deep.  (What the deep levels do to a track is the other tests'.)"""
    w, h = 512, 512
    calib = CMC.calib("ds", w, h)
    flat = np.full((h, w), 128, np.uint8)
    pts = LC.lattice(w, h, pitch=29)[:200]
    res = []
    for levels in (None, 6):
        s = _stream(gpu_ctx, oracle, w, h, levels, calib=calib)
        CMC.apply_models(s, "ds")
        plain = _stream(gpu_ctx, oracle, w, h)
        gpu_ctx.push_stereo_batch([plain, s], [flat, flat], [flat, flat])
        gpu_ctx.sync()
        r = gpu_ctx.track_batch([plain, s], [dict(pts=pts[:7], do_temporal=0), dict(pts=pts, do_temporal=0)])
        res.append(r)
        s.close()
        plain.close()
    for k in NAMES:
        assert res[0][1][k].tobytes() == res[1][1][k].tobytes(), k
        assert res[0][0][k].tobytes() == res[1][0][k].tobytes(), k
    assert np.abs(res[1][1]["out1"]).sum() > 0 and not LC.same(res[1][1]["out1"], pts)


# ------------------------------------------------------------------------------------------ forward-backward check
@_guarded
def test_forward_backward_check_on_a_deep_stream(gpu_ctx, oracle, monkeypatch):
    """The gate equals fb_reference.gate with its LK replaced by the restatement at the stream's depth, applied to the unchecked
    outputs; the restated backward track at four levels would decide otherwise for some point."""
    prev0, curr0, curr1, pts = _scene(oracle, "smooth")
    levels = 6
    s = _stream(gpu_ctx, oracle, TW, TH, levels)
    s.push_stereo(prev0, prev0)
    s.swap()
    s.push_stereo(curr0, curr1)
    r0 = s.track(pts, 1)
    _assert_track(r0, _reference(oracle, "smooth", levels, 1), len(pts), "unchecked")
    s.set_fb_check("both", 0.05, 0.05)
    r1 = s.track(pts, 1)
    s.close()
    before = [r0[k] for k in NAMES]
    monkeypatch.setattr(FB, "_lk", lambda a, b, p, g: D.lk_track(a, b, p, g, levels))
    want = FB.gate(prev0, curr0, curr1, 3, 0.05, 0.05, 1, pts, *before)
    for k, a in zip(NAMES, want):
        assert a.tobytes() == r1[k].tobytes(), k
    assert (want[4] != r0["status"]).sum() >= 3 and (want[4] != 0).sum() >= 5


# ------------------------------------------------------------------------------------------ device frame
@_guarded
def test_runner_device_frames_equal_the_phased_path(oracle):
    """A Runner with set_lk_levels(6) over a short synthetic sequence takes the one-call device frame for every frame after the
    first and publishes, bit for bit, what the same sequence gives through the phased path of the host mirror (books on the
    host)."""
    from msckf_stereo_c_amd import runner as R
    w, h, n_frames = 752, 480, 6
    syn = oracle.Synth(seed=0x5EED0042, width=w, height=h, n_static=3, motion_scale=3.0)
    frames = [syn.render(k) for k in range(n_frames)]
    runs = []
    try:
        for host in (0, 1):                           # device books (the one-call device frame), host books (the phased path)
            R.set_fe_books_on_host(host)
            r = R.Runner(syn.calib, default_fe_cfg(), default_ekf_cfg(max_cam_state_size=10), 1, 1)
            r.set_lk_levels(6)
            runs.append(r)
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
            for x, y in zip(d0[:4], d1[:4]):
                assert x.tobytes() == y.tobytes(), k
            i0, i1 = d0[4], d1[4]
            assert (i0.before_tracking, i0.after_tracking, i0.after_matching, i0.after_ransac) == (i1.before_tracking, i1.after_tracking, i1.after_matching, i1.after_ransac)
            assert len(d0[0]) > 10, k
            n_tracked += i0.after_matching
        assert runs[0].num_device_frames() == n_frames - 1 and runs[1].num_device_frames() == 0
        assert n_tracked > 10 * (n_frames - 1)
    finally:
        R.set_fe_books_on_host(-1)
    with pytest.raises(capi.MskfError):
        runs[0].set_lk_levels(5)                      # after the first push
    r = R.Runner(syn.calib, default_fe_cfg(), default_ekf_cfg(), 1, 2)
    for bad in (dict(levels=3), dict(levels=9), dict(levels=7), dict(levels=5, stream=2)):
        with pytest.raises(capi.MskfError):
            r.set_lk_levels(**bad)
    r.set_lk_levels(5, stream=1)
    r.close()
    for x in runs:
        x.close()


# ------------------------------------------------------------------------------------------ refusals
@_guarded
def test_refusals(gpu_ctx, oracle):
    L = gpu_ctx.L
    L.mskf_fe_set_lk_levels.argtypes = [C.c_void_p, C.c_int]
    L.mskf_fe_get_lk_levels.argtypes = [C.c_void_p, C.c_void_p]
    L.mskf_last_error.restype = C.c_char_p
    L.mskf_abi_version.restype = C.c_int
    assert L.mskf_abi_version() == 4
    s = _stream(gpu_ctx, oracle, 752, 480)
    assert s.get_lk_levels() == 4                                         # a stream never set
    for bad in (3, 9, 0, -1, 1 << 20):
        assert _status(s.set_lk_levels, bad) == -1 and b"4 .. 8" in L.mskf_last_error()
        assert s.get_lk_levels() == 4
    assert _status(s.set_lk_levels, 7) == -1 and b"at most 6" in L.mskf_last_error()
    assert _status(s.set_lk_levels, 8) == -1 and s.get_lk_levels() == 4
    assert L.mskf_fe_set_lk_levels(None, 5) == -1 and L.mskf_fe_get_lk_levels(s.h, None) == -1
    for good in (6, 5, 4, 6):
        s.set_lk_levels(good)
        assert s.get_lk_levels() == good
    small = _stream(gpu_ctx, oracle, 240, 120)                            # level 4 would be 15 x 8
    assert _status(small.set_lk_levels, 5) == -1 and b"at most 4" in L.mskf_last_error()
    small.set_lk_levels(4)
    small.close()
    big = _stream(gpu_ctx, oracle, 3840, 2160)
    big.set_lk_levels(8)
    assert big.get_lk_levels() == 8
    big.close()
    # a default stream serves four levels only
    d = _stream(gpu_ctx, oracle, 752, 480)
    a, b = _images(752, 480, 3)[:2]
    d.push_stereo(a, b)
    assert d.get_level(1, 3).shape == (60, 94) and _status(d.get_level, 1, 4) == -1
    assert _status(d.set_lk_levels, 5) == -1 and b"first push" in L.mskf_last_error()      # after the first push
    assert d.get_lk_levels() == 4
    # ... and never while a batch owns the front-end arenas
    s.set_lk_levels(4)
    gpu_ctx.track_batch_begin([d], [dict(pts=np.array([[40.0, 40.0], [90.0, 60.0]]), do_temporal=0)])
    try:
        assert _status(s.set_lk_levels, 5) == -1 and b"track batch" in L.mskf_last_error()
    finally:
        gpu_ctx.track_batch_end()
    assert s.get_lk_levels() == 4
    s.set_lk_levels(5)
    s.push_stereo(a, b)
    assert _status(s.set_lk_levels, 6) == -1 and s.get_lk_levels() == 5
    assert s.get_level(2, 4).shape == (30, 47) and _status(s.get_level, 2, 5) == -1
    s.close()
    d.close()
