"""k_detect_cells as a register / DPP row march, launched directly (fe_launch_detect) at the places where the march changes what
it does: widths around a strip of 56 output columns, heights around a segment of 32 rows, segments of 64 and 128 rows, cells
narrower than a lane's four columns and wider than a strip or higher than a segment, scores at the equalities of the exact
test, keys of an older generation, launches whose streams differ in size.  Everything is bit-exact against the oracle's
cell_maxima (tests/detector_cases.py says what each case is for; tests/test_detector_cases.py shows that the set would see the
mistakes it is aimed at).

A direct launch hands the kernel descriptors of its own: images in one buffer with 64 bytes of padding either side of each,
every stream's key array between guard words of value 1 (nonzero and below every key: an atomicMax that lands on a guard
changes it).  The keys  gen | score | ~order  are decoded here."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import detector_cases as DC
import detector_reference as DR
from msckf_stereo_c_amd import build, capi
from msckf_stereo_c_amd.ctypes_types import default_ekf_cfg, default_fe_cfg

from hip_runtime import Hip

pytestmark = pytest.mark.gpu

PAD = 64            # bytes in front of and behind every image
GUARD = 1           # the word in front of and behind every key array
_HIP_ERRORS = []    # after a HIP error no test of this module launches anything


class PyrDev(C.Structure):
    _fields_ = [("lvl", C.c_void_p * 4), ("w", C.c_int * 4), ("h", C.c_int * 4)]


class CamDev(C.Structure):
    _fields_ = [("K", C.c_double * 4), ("D", C.c_double * 4), ("model", C.c_int), ("pad_", C.c_int)]


class FeStreamDev(C.Structure):
    """FeStreamDev of csrc/hip/fe_device.h.  The detector reads curr0.lvl[0], curr0.w[0], curr0.h[0], det_cols, cell_w, cell_h,
    det_floor and cell_keys; everything else stays zero.  tests/cpp/fe_device_layout.cpp reports the header's own size and field
    offsets, which test_fe_stream_dev_layout_matches_the_header compares with this mirror."""
    _fields_ = [("prev0", PyrDev), ("curr0", PyrDev), ("curr1", PyrDev), ("cam0", CamDev), ("cam1", CamDev),
                ("R01", C.c_double * 9), ("E", C.c_double * 9), ("Hpred", C.c_double * 9), ("epi_thresh", C.c_double),
                ("n_pts", C.c_int), ("n_pts_dev", C.c_void_p), ("do_temporal", C.c_int),
                ("in_pts", C.c_void_p), ("out0", C.c_void_p), ("out1", C.c_void_p), ("und0", C.c_void_p), ("und1", C.c_void_p), ("status", C.c_void_p),
                ("det_rows", C.c_int), ("det_cols", C.c_int), ("cell_w", C.c_int), ("cell_h", C.c_int), ("det_floor", C.c_int),
                ("cell_keys", C.c_void_p)]


def test_fe_stream_dev_layout_matches_the_header(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    so = str(tmp_path / "libfe_device_layout.so")
    subprocess.check_call([build.HIPCC, "-O1", "-std=c++17", "-shared", "-fPIC", "-I", root, "-o", so, os.path.join(root, "tests", "cpp", "fe_device_layout.cpp")])
    L, out = C.CDLL(so), (C.c_int * 32)()
    n = L.fe_stream_dev_layout(out, 32)
    assert n == len(FeStreamDev._fields_) + 1
    assert list(out[:n]) == [C.sizeof(FeStreamDev)] + [getattr(FeStreamDev, name).offset for name, _ in FeStreamDev._fields_]
    n = L.pyr_dev_layout(out, 32)
    assert list(out[:n]) == [C.sizeof(PyrDev)] + [getattr(PyrDev, name).offset for name, _ in PyrDev._fields_]


def _decode(keys, gen, case):
    """RESULT records of a key array: a cell has a corner when its key carries this generation."""
    keys = np.asarray(keys, np.uint64)
    out = np.zeros(len(keys), DR.RESULT)
    has = (keys >> np.uint64(56)) == np.uint64(gen)
    order = (np.uint64(0xFFFFFFFF) - (keys & np.uint64(0xFFFFFFFF))).astype(np.int64)
    cells = np.arange(len(keys))
    out["has"] = has
    out["score"] = np.where(has, ((keys >> np.uint64(32)) & np.uint64(0xFFFFFF)).astype(np.int64), 0)
    out["x"] = np.where(has, cells % case.cols * case.cw + order % case.cw, 0)
    out["y"] = np.where(has, cells // case.cols * case.ch + order // case.cw, 0)
    return out


def _launch(gpu_ctx, cases, gen=1, before=None, cut=None):
    """One fe_launch_detect over one descriptor per entry of `cases` (descriptors of the same image share its pixels, every
    descriptor has a key array of its own, filled with before[j] or zeros), cut for the largest image or for `cut`.  Returns the
    key arrays after the launch and what they held before it; checks the guard words and hipGetLastError."""
    assert not _HIP_ERRORS, "an earlier launch ended with a HIP error: %s" % _HIP_ERRORS
    for c in cases:           # what keeps every access of the kernel inside the buffers
        assert c.w > 16 and c.h > 16 and c.cw * c.cols >= c.w and c.ch * c.rows >= c.h and c.cw > 0 and c.ch > 0 and 0 <= c.floor < 1 << 24
    max_w, max_h = cut or (max(c.w for c in cases), max(c.h for c in cases))
    assert all(c.w <= max_w and c.h <= max_h for c in cases)
    hip = Hip()
    f = gpu_ctx.L.fe_launch_detect
    f.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_uint, C.c_void_p]
    f.restype = None
    try:
        img_off, n_img = {}, 0
        for c in cases:
            k = (c.kind, c.w, c.h, c.seed)
            if k not in img_off:
                img_off[k] = n_img + PAD
                n_img += PAD + (c.w * c.h + 15) // 16 * 16
        n_img += PAD
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
        d_img, d_keys = hip.alloc(n_img, False), hip.alloc(8 * n_keys, False)
        hip.put(d_img, host_img)
        hip.put(d_keys, host_keys)
        desc = (FeStreamDev * len(cases))()
        for d, c, o in zip(desc, cases, key_off):
            d.curr0.lvl[0] = d_img + img_off[(c.kind, c.w, c.h, c.seed)]
            d.curr0.w[0], d.curr0.h[0] = c.w, c.h
            d.det_rows, d.det_cols, d.cell_w, d.cell_h, d.det_floor = c.rows, c.cols, c.cw, c.ch, c.floor
            d.cell_keys = d_keys + 8 * o
        raw = np.frombuffer(bytes(desc), np.uint8).copy()
        d_desc = hip.alloc(raw.size, False)
        hip.put(d_desc, raw)
        f(d_desc, len(cases), max_w, max_h, gen, gpu_ctx.hip_stream())
        gpu_ctx.sync()
        err = hip.last_error()
        assert err == 0, "hipGetLastError %d after k_detect_cells" % err
        got = hip.get(d_keys, 8 * n_keys).view(np.uint64)
        assert np.array_equal(hip.get(d_img, n_img), host_img), "the images changed"
    except BaseException as e:
        _HIP_ERRORS.append(repr(e))
        raise
    finally:
        hip.free()
    inside = np.zeros(n_keys, bool)
    for c, o in zip(cases, key_off):
        inside[o:o + c.rows * c.cols] = True
    assert np.all(got[~inside] == GUARD), "a key landed outside the key arrays: words %s" % np.flatnonzero(~inside & (got != GUARD))[:8]
    return [got[o:o + c.rows * c.cols] for c, o in zip(cases, key_off)], [host_keys[o:o + c.rows * c.cols] for c, o in zip(cases, key_off)]


def _check(oracle, cases, keys, before, gen=1):
    """Every descriptor's keys against the oracle: score, x and y of the cells that have a corner, and the key from before the
    launch, bit for bit, in the cells that have none."""
    for j, (c, k, b) in enumerate(zip(cases, keys, before)):
        got, ref = _decode(k, gen, c), DC.expected(oracle, c)
        for name in ("has", "score", "x", "y"):
            bad = np.flatnonzero(got[name] != ref[name])
            assert not len(bad), "descriptor %d (%s), %s of cell %d: %d, oracle %d (%d cells differ)" % (
                j, c.name, name, bad[0], got[name][bad[0]], ref[name][bad[0]], len(bad))
        assert np.array_equal(k[~ref["has"]], b[~ref["has"]]), "descriptor %d (%s): a cell without a corner changed" % (j, c.name)


def _run(gpu_ctx, oracle, cases, **kw):
    keys, before = _launch(gpu_ctx, cases, **kw)
    _check(oracle, cases, keys, before, kw.get("gen", 1))
    return keys


# ------------------------------------------------------------------ strip and segment seams
def test_widths_around_the_strips_in_one_launch(gpu_ctx, oracle):
    """One stream per width 17 .. 20 and 16 + 56 k - 1 .. 16 + 56 k + 4 (k = 1, 2), 40 rows each, in a launch cut for the widest:
    the last output column is the last one of a strip, the one before it, or the first ones of the next strip, and the clamped
    last load (cl = min(c0, W - 4)) is shifted by every W mod 4."""
    assert {w % 4 for w in DC.WIDTHS[4:]} == {0, 1, 2, 3}
    _run(gpu_ctx, oracle, DC.width_cases())


def test_heights_around_the_segments_in_one_launch(gpu_ctx, oracle):
    """One stream per height 17 and 16 + 32 k - 1 .. 16 + 32 k + 1 (k = 1, 2, 3), 72 columns each: the last scored row is the
    last of a 32-row segment, the one before it, or the only row of the next segment."""
    assert DR.seg_rows(len(DC.HEIGHTS), 72, max(DC.HEIGHTS)) == 32
    _run(gpu_ctx, oracle, DC.height_cases())


@pytest.mark.parametrize("which", ["first_width", "last_width", "first_height", "last_height"] + ["%dx%d" % s for s in DC.TINY])
def test_seam_sizes_alone(gpu_ctx, oracle, which):
    """The first and the last width and height of the lists and the smallest images the kernel accepts, each in a launch of its
    own (cut for that image: no switched-off job beside it).  17 x 17 has exactly one scored pixel."""
    single = {"first_width": DC.width_cases()[0], "last_width": DC.width_cases()[-1], "first_height": DC.height_cases()[0], "last_height": DC.height_cases()[-1]}
    single.update({"%dx%d" % (c.w, c.h): c for c in DC.tiny_cases()})
    case = single[which]
    keys = _run(gpu_ctx, oracle, [case])
    if (case.w, case.h) == (17, 17):
        assert (keys[0] != 0).sum() <= 1


# ------------------------------------------------------------------ cells
@pytest.mark.parametrize("kind", DC.GEOMETRY_KINDS)
def test_cell_geometries(gpu_ctx, oracle, kind):
    """137 x 89 (three strips, three segments) with cells 1 .. 7, 56, 57 and 137 columns wide and 1, 7, 8, 31, 32, 33, 65 and 89
    rows high, one stream per geometry: the per-column keys of cells under four pixels, the two-cell pass of the segmented
    maximum, several strips or several segments feeding one cell through atomicMax, one cell over the whole image."""
    cases = DC.geometry_cases(kind)
    assert {c.cw for c in cases} >= set(DC.CELL_WS) and {c.ch for c in cases} >= set(DC.CELL_HS)
    assert DR.seg_rows(len(cases), DC.GW, DC.GH) == 32
    _run(gpu_ctx, oracle, cases)


def test_cells_of_the_ceil_rule(gpu_ctx, oracle):
    """Cells 56 and 57 wide and 31, 32, 33 and 65 high as the C ABI would size them, against the oracle's own reduction."""
    cases = DC.ceil_big_cell_cases()
    assert all(c.ceil for c in cases)
    _run(gpu_ctx, oracle, cases)


@pytest.mark.parametrize("kind", list(DC.ALL_TIE) + ["tile"])
def test_one_cell_over_the_image(gpu_ctx, oracle, kind):
    """The tie-break survives the merge across strips and segments: on the images where every pixel has the same score the one
    corner is (8, 8), on the repeated tile it is the oracle's first maximum."""
    case = DC.one_cell_case(kind)
    got = _decode(_run(gpu_ctx, oracle, [case])[0], 1, case)
    if kind in DC.ALL_TIE:
        assert (got["score"][0], got["x"][0], got["y"][0]) == (DC.ALL_TIE[kind], 8, 8)


# ------------------------------------------------------------------ score arithmetic
def test_structured_images(gpu_ctx, oracle):
    """The images that sit on the equalities of the score test: constant scores with a zero discriminant, the largest score
    there is, score zero with a + c positive (abs(a - c) == X, 2 abs(b) == X: nothing may be recorded)."""
    cases = DC.structured_cases()
    keys = _run(gpu_ctx, oracle, cases)
    for c, k in zip(cases, keys):
        if c.kind in DC.ZERO_SCORE:
            assert not k.any(), c.name


def test_floor_at_the_score(gpu_ctx, oracle):
    """det_floor at the constant score of a checkerboard and one above: nothing; one below: every cell its first valid pixel."""
    cases = DC.floor_cases()
    keys = _run(gpu_ctx, oracle, cases)
    for c, k in zip(cases, keys):
        if c.floor >= DC.ALL_TIE[c.kind]:
            assert not k.any(), c.name
        else:
            got, cells = _decode(k, 1, c), np.arange(len(k))
            assert got["has"].all() and (got["score"] == DC.ALL_TIE[c.kind]).all(), c.name
            assert np.array_equal(got["x"], np.maximum(cells % c.cols * c.cw, 8)) and np.array_equal(got["y"], np.maximum(cells // c.cols * c.ch, 8)), c.name


@pytest.mark.parametrize("gen", [2, 255])
def test_stale_generations_lose(gpu_ctx, oracle, gen):
    """Every cell holds a key of the generation before with the largest score a key can carry.  The cells of the random half get
    the new key, those of the flat half keep the old one untouched."""
    case = DC.stale_case()
    stale = np.uint64(((gen - 1) << 56) | (0xFFFFFF << 32) | (0xFFFFFFFF - 5))
    ref = DC.expected(oracle, case)
    assert 0 < ref["has"].sum() < len(ref)
    keys = _run(gpu_ctx, oracle, [case], gen=gen, before=[np.full(len(ref), stale, np.uint64)])
    assert (keys[0][~ref["has"]] == stale).all()
    assert np.array_equal(keys[0], DR.merge_keys(np.full(len(ref), stale, np.uint64), DR.keys_of(ref, case.cols, case.cw, case.ch, gen)))


# ------------------------------------------------------------------ long segments
def test_long_segments(gpu_ctx, oracle):
    """72 x 4112 (one strip, 128 segments of 32 rows) under 7, 1025 and 2049 descriptors: the launcher marches segments of 32,
    64 and 128 rows.  The descriptors cycle through seven combinations of image, grid and floor (7 is coprime to 8: every
    combination meets every block-id residue), each with a key array of its own; every descriptor equals the oracle, so the three
    launches agree cell for cell."""
    combos = DC.long_cases()
    assert len({(c.kind, c.seed) for c in combos}) == 3 and {c.ch for c in combos} == {103, 64, 1} and sum(c.floor > 0 for c in combos) == 2
    launched = []
    for n in (7, 1025, 2049):
        seg = DR.seg_rows(n, DC.LONG_W, DC.LONG_H)
        launched.append(seg)
        cases = [combos[j % 7] for j in range(n)]
        keys, before = _launch(gpu_ctx, cases)
        for j in range(7):          # one comparison per combination: its descriptors' arrays stacked
            mine = np.stack(keys[j::7])
            assert (mine == mine[0]).all(), "seg_rows %d: descriptors of %s differ among themselves" % (seg, combos[j].name)
        _check(oracle, combos, keys[:7], before[:7])
        print("k_detect_cells launched with seg_rows %d (%d descriptors)" % (seg, n))
    assert launched == [32, 64, 128]


# ------------------------------------------------------------------ mixed launch, C ABI
def test_mixed_launch(gpu_ctx, oracle):
    """Eleven streams of different sizes and grids in one launch cut for the largest (200 x 130: four strips, four segments):
    switched-off jobs sit beside live ones in the same wavefront, and the stream count is no multiple of 8."""
    cases = DC.mixed_cases()
    assert len(cases) == 11 and (cases[0].w, cases[0].h) == (200, 130) == (max(c.w for c in cases), max(c.h for c in cases))
    assert any(c.w < 16 + 56 for c in cases) and any(c.h < 16 + 32 for c in cases) and any((c.w, c.h) == (17, 17) for c in cases) and any((c.w, c.h) == (200, 17) for c in cases)
    _run(gpu_ctx, oracle, cases)


def test_through_the_c_abi(gpu_ctx, oracle):
    """One mskf_fe_push_stereo_batch over nine streams of three sizes with grids of their own, twice with different images (the
    second push wins by its generation, nothing is cleared in between): cell_maxima of every stream equals the oracle."""
    streams = []
    for c in DC.abi_cases(0):
        fe = default_fe_cfg()
        fe.det_rows, fe.det_cols = c.rows, c.cols
        streams.append(capi.Stream(gpu_ctx, oracle.euroc_calib(c.w, c.h), fe, default_ekf_cfg()))
    for push in (0, 1):
        cases = DC.abi_cases(push)
        imgs = [DC.image(c.kind, c.w, c.h, c.seed) for c in cases]
        gpu_ctx.push_stereo_batch(streams, imgs, imgs)
        for s, c in zip(streams, cases):
            got, ref = s.cell_maxima(), DC.expected(oracle, c)
            assert c.ceil and len(got) == len(ref)
            for name in ("score", "x", "y"):
                assert np.array_equal(got[name].astype(np.int64), ref[name]), (c.name, name)
    for s in streams:
        s.close()
