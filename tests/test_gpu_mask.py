"""Opt-in per-camera image masks on the device (mskf_fe_set_mask; k_detect_cells<true>, k_mask_points) against the numpy
restatement of the contract (tests/mask_reference.py; DESIGN.md §3, "Image masks"), bit for bit: the masked detector launched
directly (every size, the ones the C ABI refuses as too small included) and through the ABI, the point gate launched directly
between guard bytes and behind real track calls, mixed batches, the runners, the setter's protocol and the app's YAML keys."""
import ctypes as C
import os

import numpy as np
import pytest

import detector_cases as DC
import detector_reference as DR
import mask_reference as MR
import test_mask_reference as TM
from msckf_stereo_c_amd import capi
from msckf_stereo_c_amd.ctypes_types import FeMask, default_ekf_cfg, default_fe_cfg
from test_gpu_detector_edges import FeStreamDev, _decode

from hip_runtime import Hip

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K_LK, K_FE_MASK, K_COUNT = 2, 12, 14          # MSKF_K_LK, MSKF_K_FE_MASK (the slot of MSKF_K_PT_GEOM), MSKF_K_COUNT
GUARD = 1
_HIP_ERRORS = []                              # after a HIP error no test of this module launches anything


class FeMaskDev(C.Structure):
    """FeMaskDev of csrc/hip/fe_mask.h: element i goes with descriptor i of a launch."""
    _fields_ = [("mask0", C.c_void_p), ("mask1", C.c_void_p), ("pitch_w", C.c_int), ("pad_", C.c_int)]


def test_fe_mask_dev_layout_matches_the_header(tmp_path):
    import subprocess
    so = str(tmp_path / "libfe_mask_test.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-I", ROOT, "-o", so, os.path.join(ROOT, "tests", "cpp", "fe_mask_test.cpp")])
    out = (C.c_int * 8)()
    n = C.CDLL(so).fm_mask_dev_layout(out, 8)
    assert list(out[:n]) == [C.sizeof(FeMaskDev)] + [getattr(FeMaskDev, k).offset for k in ("mask0", "mask1", "pitch_w")]


# ------------------------------------------------------------------------------------------ masks and what they should give
_scores = {}


def _score(case):
    key = (case.kind, case.w, case.h, case.seed)
    if key not in _scores:
        _scores[key] = DR.score_map(DC.image(*key))
        _scores[key].setflags(write=False)
    return _scores[key]


def mask_set(case):
    """name -> usable plane (bool) for a detector case; "half_margin5" is given as eroded here (a direct launch hands the kernel
    the plane itself; through the ABI the same plane comes from the setter's margin)."""
    h, w, cw, ch = case.h, case.w, case.cw, case.ch
    yy, xx = np.mgrid[0:h, 0:w]
    plain = DR.reduce_cells(_score(case), case.rows, case.cols, cw, ch, case.floor)
    rng = np.random.default_rng([w, h, 77])
    m = {"all_usable": np.ones((h, w), bool), "all_masked": np.zeros((h, w), bool)}
    u = np.ones((h, w), bool)
    u[plain["y"][plain["has"]], plain["x"][plain["has"]]] = False
    m["max_masked"] = u                                               # the next-best pixel of every cell must win
    m["one_per_cell"] = (yy % ch == ch // 2) & (xx % cw == cw // 2)
    m["checker"] = (xx + yy) % 2 == 0
    for k in range(4):
        m["stripe%d" % k] = xx % 4 == k                               # one bit of every lane's nibble
    m["cols32"] = ~np.isin(xx % 32, (31, 0))                          # the columns either side of a mask word's edge masked out
    m["cell_last_row"] = yy % ch != ch - 1
    m["seg_rows"] = ~np.isin((yy - DR.BORDER) % 32, (31, 0))          # the rows either side of a 32-row segment's seam
    m["rand50"] = rng.random((h, w)) >= 0.5
    m["rand01"] = rng.random((h, w)) >= 0.01
    m["half_margin5"] = MR.erode(xx >= w // 2, 5)
    return m


def _want(case, usable):
    return MR.masked_cell_maxima(_score(case), usable, case.rows, case.cols, case.cw, case.ch, case.floor)


def _same_results(got, want, what):
    for k in ("has", "score", "x", "y"):
        assert np.array_equal(got[k], want[k]), (what, k, np.flatnonzero(got[k] != want[k])[:8])


# ------------------------------------------------------------------------------------------ the masked detector, launched directly
def _launch_masked(gpu_ctx, items, gen=1, before=None):
    """One fe_launch_detect_masked over one descriptor per (case, usable plane or None = a null mask0).  Returns the key arrays."""
    assert not _HIP_ERRORS, "an earlier launch ended with a HIP error: %s" % _HIP_ERRORS
    cases = [c for c, _ in items]
    for c, u in items:           # what keeps every access of the kernel inside the buffers
        assert c.w > 16 and c.h > 16 and c.cw * c.cols >= c.w and c.ch * c.rows >= c.h and c.cw > 0 and c.ch > 0 and 0 <= c.floor < 1 << 24
        assert u is None or u.shape == (c.h, c.w)
    max_w, max_h = max(c.w for c in cases), max(c.h for c in cases)
    hip = Hip()
    f = gpu_ctx.L.fe_launch_detect_masked
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_uint, C.c_void_p]
    f.restype = None
    try:
        img_off, n_img = {}, 0
        for c in cases:
            k = (c.kind, c.w, c.h, c.seed)
            if k not in img_off:
                img_off[k] = n_img + 64
                n_img += 64 + (c.w * c.h + 15) // 16 * 16
        n_img += 64
        host_img = np.full(n_img, 0xA5, np.uint8)
        for k, o in img_off.items():
            host_img[o:o + k[1] * k[2]] = DC.image(*k).reshape(-1)
        key_off, n_keys = [], 0
        for c in cases:
            key_off.append(n_keys + 1)
            n_keys += 1 + c.rows * c.cols
        n_keys += 1
        host_keys = np.full(n_keys, GUARD, np.uint64)
        for j, (c, o) in enumerate(zip(cases, key_off)):
            host_keys[o:o + c.rows * c.cols] = 0 if before is None else before[j]
        planes = [None if u is None else MR.pack(u) for _, u in items]
        word_off, n_words = [], 0
        for p in planes:
            word_off.append(n_words)
            n_words += 0 if p is None else p.size
        host_words = np.zeros(max(n_words, 1), np.uint32)
        for p, o in zip(planes, word_off):
            if p is not None:
                host_words[o:o + p.size] = p.reshape(-1)
        d_img, d_keys, d_words = hip.alloc(n_img, False), hip.alloc(8 * n_keys, False), hip.alloc(host_words.nbytes, False)
        hip.put(d_img, host_img)
        hip.put(d_keys, host_keys)
        hip.put(d_words, host_words)
        desc, masks = (FeStreamDev * len(cases))(), (FeMaskDev * len(cases))()
        for d, m, c, o, p, wo in zip(desc, masks, cases, key_off, planes, word_off):
            d.curr0.lvl[0] = d_img + img_off[(c.kind, c.w, c.h, c.seed)]
            d.curr0.w[0], d.curr0.h[0] = c.w, c.h
            d.det_rows, d.det_cols, d.cell_w, d.cell_h, d.det_floor = c.rows, c.cols, c.cw, c.ch, c.floor
            d.cell_keys = d_keys + 8 * o
            m.mask0 = None if p is None else d_words + 4 * wo
            m.pitch_w = MR.pitch_words(c.w)
        raw_d, raw_m = np.frombuffer(bytes(desc), np.uint8).copy(), np.frombuffer(bytes(masks), np.uint8).copy()
        d_desc, d_masks = hip.alloc(raw_d.size, False), hip.alloc(raw_m.size, False)
        hip.put(d_desc, raw_d)
        hip.put(d_masks, raw_m)
        f(d_desc, d_masks, len(cases), max_w, max_h, gen, gpu_ctx.hip_stream())
        gpu_ctx.sync()
        err = hip.last_error()
        assert err == 0, "hipGetLastError %d after k_detect_cells<true>" % err
        got = hip.get(d_keys, 8 * n_keys).view(np.uint64)
        assert np.array_equal(hip.get(d_img, n_img), host_img) and np.array_equal(hip.get(d_words, host_words.nbytes).view(np.uint32), host_words)
    except BaseException as e:
        _HIP_ERRORS.append(repr(e))
        raise
    finally:
        hip.free()
    inside = np.zeros(n_keys, bool)
    for c, o in zip(cases, key_off):
        inside[o:o + c.rows * c.cols] = True
    assert np.all(got[~inside] == GUARD), "a key landed outside the key arrays"
    return [got[o:o + c.rows * c.cols] for c, o in zip(cases, key_off)]


DIRECT = ([DC.cell_grid("d17", "random", 17, 17, 4, 4, seed=1)]
          + [DC.like16("dw%d" % w, "random", w, 40, seed=w) for w in (31, 32, 33, 63, 64, 65, 97, 71, 72, 73, 74, 75)]
          + [DC.like16("dh%d" % h, "random", 72, h, seed=h) for h in (47, 48, 49)]
          + [DC.cell_grid("dnarrow33", "random", 33, 40, 3, 5, seed=5), DC.cell_grid("dnarrow73", "random", 73, 40, 3, 5, seed=6),
             DC.like16("dtile", "tile", DC.GW, DC.GH), DC.like16("dchecker8", "checker8", DC.GW, DC.GH), DC.like16("d188", "random", 188, 120, seed=9)]
          + [DC.like16("dfloor%+d" % d, "checker8", DC.GW, DC.GH, floor=DC.ALL_TIE["checker8"] + d) for d in (-1, 0, 1)])


@pytest.mark.parametrize("case", DIRECT, ids=lambda c: c.name)
def test_masked_detector_direct(gpu_ctx, case):
    """Every mask of mask_set on one image in ONE launch (a descriptor each, the last one with a null mask = unmasked)."""
    ms = mask_set(case)
    items = [(case, u) for u in ms.values()] + [(case, None)]
    keys = _launch_masked(gpu_ctx, items)
    for (name, u), k in zip(ms.items(), keys):
        _same_results(_decode(k, 1, case), _want(case, u), (case.name, name))
    plain = DR.reduce_cells(_score(case), case.rows, case.cols, case.cw, case.ch, case.floor)
    _same_results(_decode(keys[-1], 1, case), plain, (case.name, "null mask"))
    assert keys[-1].tobytes() == keys[0].tobytes()                       # all usable == not masked, bitwise
    assert not keys[1].any()                                             # all masked: no key at all


def test_masked_detector_direct_stale_generation(gpu_ctx):
    """Keys of generation 1 with the unmasked maxima (every score at least the masked one) do not survive a masked launch of
    generation 2: decoded for generation 2, the cells hold the masked maxima and nothing else."""
    case = DC.like16("dstale", "random", DC.GW, DC.GH, seed=4)
    ms = mask_set(case)
    names = ["all_masked", "max_masked", "rand50", "half_margin5"]
    before = [DR.keys_of(DR.reduce_cells(_score(case), case.rows, case.cols, case.cw, case.ch), case.cols, case.cw, case.ch, 1)] * len(names)
    keys = _launch_masked(gpu_ctx, [(case, ms[n]) for n in names], gen=2, before=before)
    for n, k, b in zip(names, keys, before):
        want = _want(case, ms[n])
        _same_results(_decode(k, 2, case), want, n)
        assert np.array_equal(k, DR.merge_keys(b, DR.keys_of(want, case.cols, case.cw, case.ch, 2)))


# ------------------------------------------------------------------------------------------ the detector through the C ABI
def _stream(ctx, oracle, w, h):
    return capi.Stream(ctx, oracle.euroc_calib(w, h), default_fe_cfg(), default_ekf_cfg())


def _abi_case(w, h, kind="random", seed=0, floor=0):
    fe = default_fe_cfg()
    return DC.ceil_grid("abi%dx%d" % (w, h), kind, w, h, fe.det_rows, fe.det_cols, floor=floor, seed=seed)


def _maxima(s, case):
    """cell_maxima() as detector_reference.RESULT records."""
    cm = s.cell_maxima()
    assert np.array_equal(cm["cell"], np.arange(case.rows * case.cols))
    out = np.zeros(len(cm), DR.RESULT)
    out["has"] = cm["score"] > 0
    out["score"], out["x"], out["y"] = cm["score"], cm["x"].astype(np.int64), cm["y"].astype(np.int64)
    return out, cm


# default 30 x 47 grid: cells 2 x 3 at 64 x 64 (the cw < 4 branch), 4 x 4 at 188 x 120, 16 x 16 at 752 x 480
ABI_SIZES = [(64, 64), (65, 64), (97, 64), (73, 70), (188, 120), (752, 480)]


@pytest.mark.parametrize("w,h", ABI_SIZES)
def test_masked_detector_through_the_abi(gpu_ctx, oracle, w, h):
    """set_mask -> push_stereo -> cell_maxima() == the restatement; get_mask() == the eroded plane."""
    case = _abi_case(w, h, seed=w)
    img = DC.image(case.kind, w, h, case.seed)
    ms = mask_set(case)
    names = list(ms) if w < 752 else ["all_usable", "max_masked", "rand50", "cols32", "half_margin5"]
    s = _stream(gpu_ctx, oracle, w, h)
    assert (case.cw < 4) == (w < 188)
    s.push_stereo(img, img)
    plain, plain_cm = _maxima(s, case)
    _same_results(plain, DR.reduce_cells(_score(case), case.rows, case.cols, case.cw, case.ch), "no mask")
    yy, xx = np.mgrid[0:h, 0:w]
    for name in names:
        if name == "half_margin5":
            s.set_mask(cam0=(xx >= w // 2), margin=5)
        else:
            s.set_mask(cam0=np.where(ms[name], 200, 0).astype(np.uint8))
        got_mask, margin = s.get_mask(0)
        assert np.array_equal(got_mask, np.where(ms[name], 255, 0)) and margin == (5 if name == "half_margin5" else 0) and s.get_mask(1)[0] is None
        s.push_stereo(img, img)
        got, cm = _maxima(s, case)
        _same_results(got, _want(case, ms[name]), (w, h, name))
        if name == "all_usable":
            assert cm.tobytes() == plain_cm.tobytes()
        if name == "all_masked":
            assert not got["has"].any()
    s.set_mask()
    s.push_stereo(img, img)
    assert _maxima(s, case)[1].tobytes() == plain_cm.tobytes()
    s.close()


def test_masked_detector_floor_and_stale_keys_through_the_abi(gpu_ctx, oracle):
    """With det_floor at the constant score of the checkerboard, one below and one above; then a masked push after an unmasked
    one of another image: no key of the earlier push survives in a cell the mask has emptied."""
    w, h = 188, 120
    tie = DC.ALL_TIE["checker8"]
    s = _stream(gpu_ctx, oracle, w, h)
    base = _abi_case(w, h, "checker8")
    usable = mask_set(base)["rand50"]
    s.set_mask(cam0=usable)
    for d in (-1, 0, 1):
        case = _abi_case(w, h, "checker8", floor=tie + d)
        s.set_detect_floor(case.floor)
        s.push_stereo(DC.image("checker8", w, h), DC.image("checker8", w, h))
        got, _ = _maxima(s, case)
        _same_results(got, _want(case, usable), d)
        assert got["has"].any() == (d < 0)
    s.set_detect_floor(0)
    s.set_mask()
    rnd = _abi_case(w, h, "random", seed=3)
    s.push_stereo(DC.image("random", w, h, 3), DC.image("random", w, h, 3))
    first, _ = _maxima(s, rnd)
    _same_results(first, DR.reduce_cells(_score(rnd), rnd.rows, rnd.cols, rnd.cw, rnd.ch), "unmasked push")
    assert first["has"].reshape(rnd.rows, rnd.cols)[:, :(w // 2) // rnd.cw].sum() > 100          # keys the masked push must not inherit
    half = mask_set(rnd)["half_margin5"]
    s.set_mask(cam0=half)
    blocks = _abi_case(w, h, "blocks", seed=4)
    s.push_stereo(DC.image("blocks", w, h, 4), DC.image("blocks", w, h, 4))
    got, _ = _maxima(s, blocks)
    _same_results(got, _want(blocks, half), "stale")
    assert not got["has"].reshape(blocks.rows, blocks.cols)[:, :(w // 2) // blocks.cw].any()
    s.close()


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
        self.ctx.L.mskf_ctx_set_timing.argtypes = [C.c_void_p, C.c_int]
        assert self.ctx.L.mskf_ctx_set_timing(self.ctx.h, 1) == 0
        _timing(self.ctx)
        return self

    def __exit__(self, *exc):
        self.launches = _timing(self.ctx)
        self.ctx.L.mskf_ctx_set_timing(self.ctx.h, 0)
        return False


# ------------------------------------------------------------------------------------------ mixed batch
def _levels(s):
    return [s.get_level(role, l) for role in (1, 2) for l in range(4)]


def test_mixed_batch(gpu_ctx, oracle):
    """push_stereo_batch and track_batch over five streams of two sizes with mask0 only, mask1 only, both, none, none: the masked
    streams equal the restatement, the unmasked ones a batch without any mask, bit for bit; the gate's timing kind is 0 for a
    batch with no masked stream and 1 with one."""
    shapes = [(188, 120), (376, 240), (188, 120), (376, 240), (188, 120)]
    which = [(True, False), (False, True), (True, True), (False, False), (False, False)]
    syn = {sh: oracle.Synth(seed=0x5EED00B0 + sh[0], width=sh[0], height=sh[1]) for sh in set(shapes)}
    pairs = [syn[sh].render(k) for k, sh in enumerate(shapes)]
    cases = [DC.ceil_grid("mix%d" % k, "random", w, h, 30, 47) for k, (w, h) in enumerate(shapes)]
    scores = [DR.score_map(p[0]) for p in pairs]

    def run(masks):
        ss = [_stream(gpu_ctx, oracle, w, h) for (w, h) in shapes]
        for s, m in zip(ss, masks):
            if m[0] is not None or m[1] is not None:
                s.set_mask(cam0=m[0], cam1=m[1])
        with _Timed(gpu_ctx) as t_push:
            gpu_ctx.push_stereo_batch(ss, [p[0] for p in pairs], [p[1] for p in pairs])
            gpu_ctx.sync()
        cms = [s.cell_maxima() for s in ss]
        lv = [_levels(s) for s in ss]
        pts = [np.stack([cm["x"][cm["score"] > 2560], cm["y"][cm["score"] > 2560]], 1)[:60] for cm in cms]
        with _Timed(gpu_ctx) as t_trk:
            res = gpu_ctx.track_batch(ss, [dict(pts=p, do_temporal=0) for p in pts])
        for s in ss:
            s.close()
        return cms, lv, pts, res, t_push.launches, t_trk.launches

    none = [(None, None)] * 5
    cm0, lv0, pts0, res0, tp0, tt0 = run(none)
    assert tp0[K_FE_MASK] == 0 and tt0[K_FE_MASK] == 0 and tt0[K_LK] == 1
    assert all(len(p) > 10 for p in pts0) and all((r["status"] == 3).sum() > 5 for r in res0)
    # masks cut from the unmasked results: cam0 under every third candidate, cam1 under every fifth match
    masks = []
    for (w, h), (m0, m1), p, r in zip(shapes, which, pts0, res0):
        u0, u1 = np.ones((h, w), bool), np.ones((h, w), bool)
        u0[MR.pixel(p[::3, 1]), MR.pixel(p[::3, 0])] = False
        ok = np.flatnonzero(r["status"] == 3)[::5]
        u1[MR.pixel(r["out1"][ok, 1]), MR.pixel(r["out1"][ok, 0])] = False
        masks.append((u0 if m0 else None, u1 if m1 else None))
    cm1, lv1, pts1, res1, tp1, tt1 = run(masks)
    assert tp1[K_FE_MASK] == 0 and tt1[K_FE_MASK] == 1 and tt1[K_LK] == 1
    for k, (case, (u0, u1)) in enumerate(zip(cases, masks)):
        for a, b in zip(lv0[k], lv1[k]):
            assert a.tobytes() == b.tobytes()
        if u0 is None:
            assert cm1[k].tobytes() == cm0[k].tobytes() and np.array_equal(pts1[k], pts0[k])
        else:
            want = MR.masked_cell_maxima(scores[k], u0, case.rows, case.cols, case.cw, case.ch)
            assert np.array_equal(cm1[k]["score"], want["score"]) and np.array_equal(cm1[k]["x"][want["has"]], want["x"][want["has"]])
            assert cm1[k].tobytes() != cm0[k].tobytes()
        if u0 is None:
            # the same input points: the gate is a pure function of the unmasked track's outputs
            w, h = shapes[k]
            want = MR.gate(None, None if u1 is None else MR.pack(u1), w, h, res0[k]["out0"], res0[k]["out1"], res0[k]["und0"], res0[k]["und1"], res0[k]["status"])
            for name, a in zip(("out0", "out1", "und0", "und1", "status"), want):
                assert a.tobytes() == res1[k][name].tobytes(), (k, name)
            if u1 is None:
                assert all(res0[k][n].tobytes() == res1[k][n].tobytes() for n in res0[k])
            else:
                assert (res1[k]["status"] != res0[k]["status"]).any()


# ------------------------------------------------------------------------------------------ the gate, launched directly
GW_, GH_ = TM.W, TM.H


def _gate_direct(gpu_ctx, max_pts):
    """One fe_launch_mask_points over descriptors with n = 0, 1, 63, 64, 65, 257 points and both masks, 65 points with mask0 only,
    mask1 only and no mask, and 257 points of which a device-side count admits 100.  Every array lies between guard bytes in one
    buffer, which is compared whole with the restatement's."""
    assert not _HIP_ERRORS, "an earlier launch ended with a HIP error: %s" % _HIP_ERRORS
    m0, m1 = TM.gate_masks()
    base = TM.gate_points()
    specs = [(n, True, True, None) for n in (0, 1, 63, 64, 65, 257)] + [(65, True, False, None), (65, False, True, None), (65, False, False, None), (257, True, True, 100)]
    hip = Hip()
    f = gpu_ctx.L.fe_launch_mask_points
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    f.restype = None
    try:
        offs, total = [], 64
        for n, _, _, _ in specs:
            o = {}
            for name, size in (("out0", 8 * n), ("out1", 8 * n), ("und0", 8 * n), ("und1", 8 * n), ("status", n), ("count", 4)):
                o[name] = total
                total += (size + 63) // 64 * 64 + 64
            offs.append(o)
        host, want = np.full(total, 0xA5, np.uint8), np.full(total, 0xA5, np.uint8)
        changed = 0
        for k, ((n, use0, use1, count), o) in enumerate(zip(specs, offs)):
            idx = (np.arange(n) * 7 + k) % len(base[4])
            arrs = [a[idx].copy() for a in base]
            m = n if count is None else count
            gated = MR.gate(m0 if use0 else None, m1 if use1 else None, GW_, GH_, *[a[:m] for a in arrs])
            exp = [np.concatenate([g, a[m:]]) for g, a in zip(gated, arrs)]
            changed += int((exp[4] != arrs[4]).sum())
            for name, a, e in zip(("out0", "out1", "und0", "und1", "status"), arrs, exp):
                host[o[name]:o[name] + a.nbytes] = a.reshape(-1).view(np.uint8)
                want[o[name]:o[name] + e.nbytes] = e.reshape(-1).view(np.uint8)
            cnt = np.array([0 if count is None else count], np.int32).view(np.uint8)
            host[o["count"]:o["count"] + 4] = cnt
            want[o["count"]:o["count"] + 4] = cnt
        assert changed > 50
        words = np.concatenate([m0.reshape(-1), m1.reshape(-1)])
        d_buf, d_words = hip.alloc(total, False), hip.alloc(words.nbytes, False)
        hip.put(d_buf, host)
        hip.put(d_words, words)
        desc, masks = (FeStreamDev * len(specs))(), (FeMaskDev * len(specs))()
        for d, m, (n, use0, use1, count), o in zip(desc, masks, specs, offs):
            d.curr0.w[0], d.curr0.h[0], d.curr1.w[0], d.curr1.h[0] = GW_, GH_, GW_, GH_
            d.n_pts = n
            d.n_pts_dev = None if count is None else d_buf + o["count"]
            d.out0, d.out1, d.und0, d.und1, d.status = (d_buf + o[k] for k in ("out0", "out1", "und0", "und1", "status"))
            m.mask0 = d_words if use0 else None
            m.mask1 = d_words + m0.nbytes if use1 else None
            m.pitch_w = MR.pitch_words(GW_)
        raw_d, raw_m = np.frombuffer(bytes(desc), np.uint8).copy(), np.frombuffer(bytes(masks), np.uint8).copy()
        d_desc, d_masks = hip.alloc(raw_d.size, False), hip.alloc(raw_m.size, False)
        hip.put(d_desc, raw_d)
        hip.put(d_masks, raw_m)
        f(d_desc, d_masks, len(specs), max_pts, gpu_ctx.hip_stream())
        gpu_ctx.sync()
        err = hip.last_error()
        assert err == 0, "hipGetLastError %d after k_mask_points" % err
        got = hip.get(d_buf, total)
        assert np.array_equal(hip.get(d_words, words.nbytes).view(np.uint32), words)
    except BaseException as e:
        _HIP_ERRORS.append(repr(e))
        raise
    finally:
        hip.free()
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "bytes %s differ from the restatement (guards and untouched fields included)" % bad[:16]


@pytest.mark.parametrize("max_pts", [257, 4])
def test_gate_direct(gpu_ctx, max_pts):
    """max_pts = 257: a lane per point; 4: the launch is cut from an estimate below the counts, a block takes several point groups."""
    _gate_direct(gpu_ctx, max_pts)


# ------------------------------------------------------------------------------------------ the gate behind a real track
@pytest.mark.parametrize("do_temporal", [1, 0])
def test_gate_behind_a_real_track(gpu_ctx, oracle, do_temporal):
    w, h = 188, 120
    syn = oracle.Synth(seed=0x5EED00C0, width=w, height=h)
    s = _stream(gpu_ctx, oracle, w, h)
    s.push_stereo(*syn.render(30))
    cm = s.cell_maxima()
    pts = np.stack([cm["x"], cm["y"]], 1)[cm["score"] > 2560][:200]
    assert len(pts) > 40
    if do_temporal:
        s.swap()
        s.push_stereo(*syn.render(31))
    with _Timed(gpu_ctx) as t0:
        r0 = s.track(pts, do_temporal)
    assert t0.launches[K_FE_MASK] == 0 and t0.launches[K_LK] == 1
    alive, matched = np.flatnonzero(r0["status"] & 1), np.flatnonzero(r0["status"] == 3)
    assert len(alive) > 30 and len(matched) > 20
    u0, u1 = np.ones((h, w), bool), np.ones((h, w), bool)
    u0[MR.pixel(r0["out0"][alive[::3], 1]), MR.pixel(r0["out0"][alive[::3], 0])] = False
    u1[MR.pixel(r0["out1"][matched[::5], 1]), MR.pixel(r0["out1"][matched[::5], 0])] = False
    s.set_mask(cam0=u0, cam1=u1)
    with _Timed(gpu_ctx) as t1:
        r1 = s.track(pts, do_temporal)
    assert t1.launches[K_FE_MASK] == 1 and t1.launches[K_LK] == 1
    want = MR.gate(MR.pack(u0), MR.pack(u1), w, h, r0["out0"], r0["out1"], r0["und0"], r0["und1"], r0["status"])
    for name, a in zip(("out0", "out1", "und0", "und1", "status"), want):
        assert a.tobytes() == r1[name].tobytes(), name
    assert (r1["status"][alive[::3]] == 0).all() and ((r1["status"] == 1) & (r0["status"] == 3)).any()
    s.set_mask()
    r2 = s.track(pts, do_temporal)
    assert all(r0[n].tobytes() == r2[n].tobytes() for n in r0)
    s.close()


# ------------------------------------------------------------------------------------------ protocol
def _status(call, *a, **kw):
    try:
        call(*a, **kw)
        return 0
    except capi.MskfError as e:
        return e.code


def test_set_mask_protocol(gpu_ctx, oracle):
    """Every refusal leaves the previous mask in force (get_mask); the setter is refused while a track batch or a device frame of
    the context is pending (the message names it) and accepted after its _end; both planes None = off."""
    w, h = 188, 120
    L = gpu_ctx.L
    L.mskf_fe_set_mask.argtypes = [C.c_void_p, C.c_void_p]
    syn = oracle.Synth(seed=0x5EED00D0, width=w, height=h)
    a, b = syn.render(0)
    s = _stream(gpu_ctx, oracle, w, h)
    assert s.get_mask(0) == (None, 0) and s.get_mask(1) == (None, 0)
    src0, src1 = TM.random_mask(w, h, 0.01, 3), TM.random_mask(w, h, 0.01, 4)
    s.set_mask(src0, src1, margin=3)
    e0, e1 = np.where(MR.erode(src0, 3), 255, 0), np.where(MR.erode(src1, 3), 255, 0)

    def unchanged():
        (g0, m0), (g1, m1) = s.get_mask(0), s.get_mask(1)
        return np.array_equal(g0, e0) and np.array_equal(g1, e1) and m0 == m1 == 3
    assert unchanged()
    plane = np.ascontiguousarray(src0)
    for bad in [FeMask(plane.ctypes.data, None, w + 1, h, w + 1, 0), FeMask(plane.ctypes.data, None, w, h - 1, w, 0), FeMask(plane.ctypes.data, None, w, h, w - 1, 0),
                FeMask(plane.ctypes.data, None, w, h, w, -1), FeMask(None, plane.ctypes.data, w, h, w, 65)]:
        assert L.mskf_fe_set_mask(s.h, C.byref(bad)) == -1 and len(L.mskf_last_error()) > 0
        assert unchanged()
    assert L.mskf_fe_set_mask(s.h, None) == -1 and L.mskf_fe_set_mask(None, None) == -1 and unchanged()
    assert _status(s.set_mask, np.ones((h, w + 2), np.uint8)) == -1 and unchanged()
    # margin 64 is the limit; a padded plane is read with its pitch
    padded = np.full((h, w + 9), 0, np.uint8)
    padded[:, :w] = src1
    assert L.mskf_fe_set_mask(s.h, C.byref(FeMask(None, padded.ctypes.data, w, h, w + 9, 64))) == 0
    g1, m1 = s.get_mask(1)
    assert s.get_mask(0)[0] is None and m1 == 64 and np.array_equal(g1, np.where(MR.erode(src1, 64), 255, 0))
    s.set_mask(src0, src1, margin=3)
    # pending track batch
    s.push_stereo(a, b)
    gpu_ctx.track_batch_begin([s], [dict(pts=np.array([[40.0, 40.0], [90.0, 60.0]]), do_temporal=0)])
    try:
        assert _status(s.set_mask, src1) == -1 and b"track batch" in L.mskf_last_error()
        assert _status(s.set_mask) == -1
    finally:
        gpu_ctx.track_batch_end()
    assert unchanged()
    # pending device frame: refused, then accepted after its _end
    s.swap()
    s.set_grid()
    gpu_ctx.frame_batch_begin([s], [(a, b)], [{}])
    try:
        assert _status(s.set_mask, src1) == -1 and b"device frame" in L.mskf_last_error()
    finally:
        gpu_ctx.frame_batch_end()
    assert unchanged()
    s.set_mask(src1)
    assert np.array_equal(s.get_mask(0)[0], np.where(src1 != 0, 255, 0)) and s.get_mask(1)[0] is None
    s.set_mask()
    assert s.get_mask(0) == (None, 0) and s.get_mask(1) == (None, 0)
    s.close()


# ------------------------------------------------------------------------------------------ runners
_RUN = dict(w=188, h=120, n_frames=30, seed=0x5EED00E0, margin=5)


def _runner_masks():
    w, h = _RUN["w"], _RUN["h"]
    m0, m1 = np.ones((h, w), np.uint8), np.ones((h, w), np.uint8)
    m0[2 * h // 3:, :] = 0            # the bottom third of cam0: a bonnet
    m1[:, :30] = 0                    # a left band of cam1
    return m0, m1


def _same_run(a, b):
    for x, y in zip(a.dump(0)[:4], b.dump(0)[:4]):
        assert np.array_equal(x, y)
    pa, pb = a.poses(0), b.poses(0)
    assert len(pa) == len(pb) > 5
    assert np.array_equal(pa["t"], pb["t"]) and np.array_equal(pa["p"], pb["p"]) and np.array_equal(pa["q"], pb["q"])
    assert np.array_equal(a.cov(0), b.cov(0))


def _sequence_run(oracle, syn, keep, pipelined=False, setup=None):
    from msckf_stereo_c_amd import runner as R
    from test_gpu_system import _attach_sequences
    run = R.Runner(syn.calib, default_fe_cfg(), default_ekf_cfg(max_cam_state_size=10), 1, 1, host_threads=1)
    if setup:
        setup(run)
    _attach_sequences(oracle, run, [syn], _RUN["n_frames"], keep)
    run.run(0, _RUN["n_frames"], threaded=True, pipelined=pipelined)
    return run


def test_runner_all_usable_and_off_again_equal_no_mask(oracle):
    syn = oracle.Synth(seed=_RUN["seed"], width=_RUN["w"], height=_RUN["h"])
    keep = []
    ones = np.ones((_RUN["h"], _RUN["w"]), np.uint8)
    plain = _sequence_run(oracle, syn, keep)
    usable = _sequence_run(oracle, syn, keep, setup=lambda r: r.set_mask(ones, ones, margin=7))

    def on_off(r):
        r.set_mask(*_runner_masks(), margin=2)
        r.set_mask()
    off = _sequence_run(oracle, syn, keep, setup=on_off)
    assert len(plain.dump(0)[0]) > 10
    _same_run(usable, plain)
    _same_run(off, plain)
    for r in (plain, usable, off):
        r.close()


def test_runner_masked(oracle):
    """Bottom third of cam0 and a left band of cam1 masked out (margin 5): every published feature of every frame lies on usable
    pixels of both cameras, every frame publishes features and every frame after the first is a device frame; pipelined ==
    lockstep == the frame-by-frame run, device books == host books, bit for bit."""
    from msckf_stereo_c_amd import runner as R
    w, h, n_frames, margin = _RUN["w"], _RUN["h"], _RUN["n_frames"], _RUN["margin"]
    syn = oracle.Synth(seed=_RUN["seed"], width=w, height=h)
    m0, m1 = _runner_masks()
    e0, e1 = MR.erode(m0, margin), MR.erode(m1, margin)
    p0, p1 = MR.pack(e0), MR.pack(e1)
    # the usable part of cam0 has texture (CPU): cells above the detector threshold in frames 0 and n_frames - 1
    fe = default_fe_cfg()
    for k in (0, n_frames - 1):
        cw, ch = DR.ceil_cells(w, h, fe.det_rows, fe.det_cols)
        assert MR.masked_cell_maxima(DR.score_map(syn.render(k)[0]), e0, fe.det_rows, fe.det_cols, cw, ch, fe.fast_threshold * 256)["has"].sum() > 50
    ekf = default_ekf_cfg(max_cam_state_size=10)
    runs = []
    try:
        for host in (0, 1):
            R.set_fe_books_on_host(host)
            r = R.Runner(syn.calib, fe, ekf, 1, 1)
            r.set_mask(m0, m1, margin=margin)
            runs.append(r)
        j, lost_somewhere = 0, False
        for k in range(n_frames):
            t_img = syn.frame_time(k)
            while True:
                s = syn.imu(j)
                j += 1
                for r in runs:
                    r.imu(0, s)
                if not (s.time_stamp <= t_img):
                    break
            a, b = syn.render(k)
            for host, r in zip((0, 1), runs):
                R.set_fe_books_on_host(host)
                r.step([a], [b], [t_img])
            ids, life, c0, c1, info = runs[0].dump(0)
            assert len(ids) >= 1, k
            assert MR.lookup(p0, w, h, MR.pixel(c0["x"]), MR.pixel(c0["y"])).all(), k
            assert MR.lookup(p1, w, h, MR.pixel(c1["x"]), MR.pixel(c1["y"])).all(), k
            assert (c0["y"] < 2 * h // 3).all() and (c1["x"] >= 30 - 0.5).all()
            for x, y in zip(runs[0].dump(0)[:4], runs[1].dump(0)[:4]):
                assert np.array_equal(x, y), k
            i1 = runs[1].dump(0)[4]
            assert (info.before_tracking, info.after_tracking, info.after_matching, info.after_ransac) == (i1.before_tracking, i1.after_tracking, i1.after_matching, i1.after_ransac)
        assert runs[0].num_device_frames() == n_frames - 1 and runs[1].num_device_frames() == 0
        pa, pb = runs[0].poses(0), runs[1].poses(0)
        assert len(pa) == len(pb) > 5 and np.array_equal(pa["p"], pb["p"]) and np.array_equal(pa["q"], pb["q"])
    finally:
        R.set_fe_books_on_host(-1)
    keep = []
    for pipelined in (False, True):
        run = _sequence_run(oracle, syn, keep, pipelined=pipelined, setup=lambda r: r.set_mask(m0, m1, margin=margin))
        _same_run(run, runs[0])
        run.close()
    # ... and the masks matter: the unmasked run publishes features where the masked one may not
    plain = _sequence_run(oracle, syn, keep)
    c0 = plain.dump(0)[2]
    assert (c0["y"] >= 2 * h // 3).any()
    plain.close()
    for r in runs:
        r.close()


def test_runner_set_mask_refuses_bad_arguments(oracle):
    from msckf_stereo_c_amd import runner as R
    syn = oracle.Synth(seed=1, width=188, height=120)
    run = R.Runner(syn.calib, default_fe_cfg(), default_ekf_cfg(), 1, 2)
    ones = np.ones((120, 188), np.uint8)
    for bad in [dict(cam0=np.ones((120, 187), np.uint8)), dict(cam0=ones, margin=65), dict(cam0=ones, margin=-1), dict(cam0=ones, stream=2),
                dict(cam0=ones, cam1=np.ones((119, 188), np.uint8))]:
        with pytest.raises(capi.MskfError):
            run.set_mask(**bad)
    run.set_mask(ones, stream=1)
    run.set_mask()
    run.close()


# ------------------------------------------------------------------------------------------ the app
def _write_pgm(path, img):
    with open(path, "wb") as f:
        f.write(b"P5\n%d %d\n255\n" % (img.shape[1], img.shape[0]))
        f.write(np.ascontiguousarray(img, dtype=np.uint8).tobytes())


def test_app_reads_mask_keys(tmp_path, oracle):
    """The headless app with mask_cam0 / mask_cam1 / mask_margin in its app_imgproc.yaml (PGM files) writes the poses of a Runner of
    one with the same masks (pose_out.txt has six decimals) and logs its tracking counts, which are not those of a Runner without
    masks; a mask file of the wrong size ends the run with the file's name in the message."""
    import shutil
    import subprocess
    from PIL import Image
    from msckf_stereo_c_amd import build
    from msckf_stereo_c_amd import runner as R
    from msckf_stereo_c_amd.ctypes_types import Calib, EkfCfg, FeCfg, ImuSample
    build.build_all()
    n_frames, w, h = 30, 752, 480
    syn = oracle.Synth(seed=0x5EED0042, width=w, height=h, n_static=21, motion_scale=3.0)
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
    m0, m1 = np.full((h, w), 255, np.uint8), np.full((h, w), 255, np.uint8)
    m0[2 * h // 3:, :] = 0
    m1[:, :100] = 0
    _write_pgm(tmp_path / "mask0.pgm", m0)
    _write_pgm(tmp_path / "mask1.pgm", m1)
    _write_pgm(tmp_path / "small.pgm", m0[:-1])
    exe = os.path.join(ROOT, "msckf_stereo_c_amd", "_build", "run_euroc_single_thread")

    def app(tag, keys):
        cfg = tmp_path / tag / "config"
        shutil.copytree(os.path.join(ROOT, "config"), cfg)
        with open(cfg / "app_imgproc.yaml", "a") as f:
            f.write("\n" + keys)
        work = tmp_path / tag / "build"
        work.mkdir()
        return subprocess.run([exe, str(mav0)], cwd=work, capture_output=True, text=True, timeout=120), work, cfg
    res, work, cfg = app("bad", "mask_cam0: %s\n" % (tmp_path / "small.pgm"))
    assert res.returncode != 0 and "small.pgm" in res.stderr
    res, work, cfg = app("good", "mask_cam0: %s\nmask_cam1: %s\nmask_margin: 5\n" % (tmp_path / "mask0.pgm", tmp_path / "mask1.pgm"))
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    got = np.loadtxt(work / "pose_out.txt").reshape(-1, 8)

    def stamp(ns):          # what the app parses: seconds * 1e9 + nanoseconds in double
        return (int(str(ns)[:-9]) * 1e9 + int(str(ns)[-9:])) * 1e-9
    imu = []
    for line in lines[1:]:
        f = line.split(",")
        v = [float(np.float32(x)) for x in f[1:7]]
        imu.append(ImuSample(stamp(int(f[0])), (C.c_double * 3)(*v[:3]), (C.c_double * 3)(*v[3:])))
    calib, fe, ekf = Calib(), FeCfg(), EkfCfg()
    assert R.lib().mskfh_load_configs(str(cfg).encode(), C.byref(calib), C.byref(fe), C.byref(ekf)) == 0

    def runner_poses(masked):
        run = R.Runner(calib, fe, ekf, 1, 1)
        if masked:
            run.set_mask(m0, m1, margin=5)
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
    last = (work / "debug_imageprocessor.txt").read_text().strip().splitlines()[-1]
    assert tuple(int(v) for v in last.split(":")[1].split(",")) == info != info_off
    assert len(got) == len(want) > 5
    assert np.abs(got[:, 0] - want["t"]).max() < 2e-6
    assert np.abs(got[:, 1:4] - want["p"]).max() <= 0.5e-6 + 1e-9 and np.abs(got[:, 4:8] - want["q"]).max() <= 0.5e-6 + 1e-9
