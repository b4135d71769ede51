"""The equalisation contract ("Equalisation") on the CPU: known answers of the numpy restatement
(tests/equalize_reference.py), and csrc/hip/fe_equalize.h (the header the kernels run) compiled with g++ == the restatement,
byte for byte, over a set of images that three deliberate mistakes in the restatement each change."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import equalize_reference as ER

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(16, 16), (40, 24), (67, 45), (188, 120), (333, 251), (752, 480)]       # w, h
TILES = [(1, 1), (2, 3), (5, 4), (8, 8)]
CLIPS = [0.0, 1.0, 3.0, 40.0]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("fe_equalize") / "libfe_equalize_test.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-shared", "-fPIC", "-I", ROOT, "-o", so,
                           os.path.join(ROOT, "tests", "cpp", "fe_equalize_test.cpp")])
    L = C.CDLL(so)
    L.eq_run.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_void_p]

    class H:
        lib = L

        @staticmethod
        def run(img, mode, tiles=(1, 1), clip_limit=0.0, want_luts=False):
            img = np.ascontiguousarray(img, dtype=np.uint8)
            h, w = img.shape
            dst = np.zeros_like(img)
            luts = np.zeros((tiles[1], tiles[0], 256), np.uint8)
            assert L.eq_run(mode, img.ctypes.data, dst.ctypes.data, w, h, tiles[0], tiles[1], float(clip_limit), luts.ctypes.data) == 0
            return (dst, luts) if want_luts else dst
    return H


def both(harness, img, mode, tiles=(1, 1), clip_limit=0.0):
    """The restatement's output, after checking that the header's is the same."""
    a = ER.equalize(img, mode, tiles, clip_limit)
    b = harness.run(img, mode, tiles, clip_limit)
    assert np.array_equal(a, b)
    return a


# ------------------------------------------------------------------------------------------ known answers, global mode
def test_global_constant_image_unchanged(harness):
    img = np.full((16, 16), 93, np.uint8)
    assert np.array_equal(both(harness, img, 1), img)


def test_global_two_levels_map_to_0_and_255(harness):
    img = np.full((24, 40), 50, np.uint8)
    img[5:, 7:] = 180
    out = both(harness, img, 1)
    assert np.array_equal(out, np.where(img == 50, 0, 255))


def test_global_ramp_lut(harness):
    """16 x 16, column x holds 16 x: sixteen levels of sixteen pixels.  i0 = 0, scale = 255 / 240 = 1.0625 exactly, the
    running sum behind bin 0 at level 16 k is 16 k: lut[16 k] = 17 k.  And the ramp of all 256 values once: scale = 255 / 255,
    lut[i] = i."""
    img = np.tile((16 * np.arange(16)).astype(np.uint8), (16, 1))
    assert np.array_equal(both(harness, img, 1), np.tile((17 * np.arange(16)).astype(np.uint8), (16, 1)))
    img = np.arange(256, dtype=np.uint8).reshape(16, 16)
    assert np.array_equal(both(harness, img, 1), img)


# ------------------------------------------------------------------------------------------ known answers, CLAHE
def _levels(shape, counts):
    """An image of the given shape with counts[v] pixels of value v, in row-major order."""
    flat = np.concatenate([np.full(n, v, np.uint8) for v, n in sorted(counts.items())])
    return flat.reshape(shape)


def _expect(img, lut):
    return np.vectorize(lut.get)(img).astype(np.uint8)


def test_clahe_one_bin_over_the_clip(harness):
    """16 x 16, one tile, T = 256, clip_limit 64 -> clip 64.  Bin 10 holds 100 (36 over), bins 20 / 30 / 40 hold 52:
    clipped = 36, nothing for every bin, residual 36, step 256 // 36 = 7: bins 0, 7, .., 245 get one each.
    Cumulative sums: at 10: 64 + 2 (bins 0, 7) = 66; at 20: 116 + 3 = 119; at 30: 168 + 5 = 173; at 40: 220 + 6 = 226.
    lutScale = 255 / 256: 65.74 -> 66, 118.54 -> 119, 172.32 -> 172, 225.12 -> 225."""
    img = _levels((16, 16), {10: 100, 20: 52, 30: 52, 40: 52})
    hist, clipped = ER.clip_and_redistribute(np.bincount(img.reshape(-1), minlength=256), ER.clip_of(64.0, 256))
    assert clipped == 36 and hist[10] == 64 and hist[0] == 1 and hist[245] == 1 and hist[252] == 0 and sum(hist) == 256
    assert np.array_equal(both(harness, img, 2, (1, 1), 64.0), _expect(img, {10: 66, 20: 119, 30: 172, 40: 225}))


def test_clahe_residual_0_and_255(harness):
    """32 x 32, one tile, T = 1024, clip_limit 128 -> clip 512.
    768 of level 100 + 256 of level 200: clipped = 256, every bin gets 1, residual 0: cum(100) = 512 + 101 = 613 -> 152.65 -> 153,
    cum(200) = 613 + 256 + 100 = 969 -> 241.30 -> 241.
    767 of level 100 + 257 of level 200: clipped = 255, residual 255, step = max(256 // 255, 1) = 1: bins 0 .. 254 get one:
    cum(100) = 613 -> 153, cum(200) = 512 + 257 + 201 = 970 -> 241.55 -> 242."""
    a = _levels((32, 32), {100: 768, 200: 256})
    assert ER.clip_and_redistribute(np.bincount(a.reshape(-1), minlength=256), 512)[1] == 256
    assert np.array_equal(both(harness, a, 2, (1, 1), 128.0), _expect(a, {100: 153, 200: 241}))
    b = _levels((32, 32), {100: 767, 200: 257})
    hist, clipped = ER.clip_and_redistribute(np.bincount(b.reshape(-1), minlength=256), 512)
    assert clipped == 255 and hist[254] == 1 and hist[255] == 0
    assert np.array_equal(both(harness, b, 2, (1, 1), 128.0), _expect(b, {100: 153, 200: 242}))


def test_clahe_step_1(harness):
    """16 x 16, T = 256, clip_limit 1 -> clip max(int(1.0), 1) = 1.  Sixteen levels 16 k of sixteen pixels: clipped = 16 * 15 = 240,
    240 // 256 = 0 for every bin, residual 240, step = max(256 // 240, 1) = 1: bins 0 .. 239 get one.
    cum(16 k) = (k + 1) + min(16 k + 1, 240): 17 k + 2 up to k = 14, 256 at k = 15.  Times 255 / 256 (exact in float):
    k = 0: 1.99 -> 2, k = 1: 18.93 -> 19, k = 8: 137.46 -> 137, k = 14: 239.06 -> 239, k = 15: 255 exactly."""
    img = np.tile((16 * np.arange(16)).astype(np.uint8), (16, 1))
    want = {16 * k: int(np.rint(((k + 1) + min(16 * k + 1, 240)) * 255.0 / 256.0)) for k in range(16)}
    assert [want[16 * k] for k in (0, 1, 8, 14, 15)] == [2, 19, 137, 239, 255]
    assert np.array_equal(both(harness, img, 2, (1, 1), 1.0), _expect(img, want))


def test_clahe_clip_limit_0_is_plain_tile_equalisation(harness):
    """No clip: lut = rint(cum * 255 / T).  16 x 16 with 64 pixels each of 0, 85, 170, 255: 63.75 -> 64, 127.5 -> 128 (half to
    even), 191.25 -> 191, 255."""
    img = _levels((16, 16), {0: 64, 85: 64, 170: 64, 255: 64})
    assert np.array_equal(both(harness, img, 2, (1, 1), 0.0), _expect(img, {0: 64, 85: 128, 170: 191, 255: 255}))


def test_clahe_geometry_known_answers(harness):
    L = harness.lib
    tw, th = C.c_int(), C.c_int()
    for (w, h, tx, ty), want in {(64, 64, 8, 8): (8, 8), (67, 45, 5, 4): (14, 12), (64, 8, 5, 4): (13, 3), (64, 4, 5, 4): (13, 2),
                                 (40, 24, 8, 8): (5, 3), (40, 25, 8, 8): (6, 4), (752, 480, 8, 8): (94, 60), (188, 120, 5, 4): (38, 31)}.items():
        L.eq_tile_size(w, h, tx, ty, C.byref(tw), C.byref(th))
        assert (tw.value, th.value) == want == ER.tile_geometry(w, h, tx, ty), (w, h, tx, ty)
    # rows: REFLECT_101 up to 2 h - 2, folded again beyond; h = 8 rows 8 .. 11, h = 4 rows 4 .. 7 (the formula as written gives h - 1 at r = 2 h - 2 = 6 already, and 7 lies beyond)
    assert [L.eq_row(r, 8) for r in range(8, 12)] == [6, 5, 4, 3] == [ER.reflect_row(r, 8) for r in range(8, 12)]
    assert [L.eq_row(r, 4) for r in range(4, 8)] == [2, 1, 3, 2] == [ER.reflect_row(r, 4) for r in range(4, 8)]
    assert [L.eq_row(r, 1) for r in range(0, 3)] == [0, 0, 0]
    assert [L.eq_col(c, 64) for c in (63, 64, 65)] == [63, 62, 61] == [ER.reflect_col(c, 64) for c in (63, 64, 65)]


@pytest.mark.parametrize("w,h,tiles,rows", [
    (67, 45, (5, 4), list(range(45)) + [43, 42, 41]),                  # both dimensions ragged
    (64, 8, (5, 4), list(range(8)) + [6, 5, 4, 3]),                    # divisible height, ragged width: a whole extra row of tiles
    (64, 4, (5, 4), list(range(4)) + [2, 1, 3, 2]),                    # ... whose last row index 7 exceeds 2 h - 2 = 6: the rule folds again
    (64, 45, (4, 4), list(range(45)) + [43, 42, 41]),                  # ragged height, divisible width: a whole extra column of tiles
])
def test_clahe_extension_equals_the_extended_image(harness, w, h, tiles, rows):
    """The virtual extension written out by hand: CLAHE of the image == CLAHE of the explicitly extended image (whose size the
    tiles divide, so that it is not extended again), cropped.  (64 x 8 with tiles 5 x 4 reaches row 11 <= 2 h - 2 = 14; the
    64 x 4 case is the one whose extended row index exceeds 2 h - 2.)"""
    img = ER.structured_images(w, h, seed=3)["random"]
    tw, th = ER.tile_geometry(w, h, *tiles)
    cols = list(range(w)) + [w - 2 - k for k in range(tw * tiles[0] - w)]
    assert len(rows) == th * tiles[1] and len(cols) == tw * tiles[0] and len(cols) > w
    ext = img[np.ix_(rows, cols)]
    for clip in (0.0, 3.0):
        assert np.array_equal(both(harness, img, 2, tiles, clip), both(harness, ext, 2, tiles, clip)[:h, :w])


def test_region_cuts_agree_with_the_pixel_formula(harness):
    """eq_axis_first (where the apply kernel cuts its regions) == the first position whose own tile index reaches k."""
    L = harness.lib
    for t in list(range(1, 70)) + [94, 128, 333, 752, 1024]:
        for n_tiles in (1, 3, 8):
            limit = t * n_tiles
            t1 = [L.eq_t1(p, t) for p in range(limit)]
            assert t1 == sorted(t1) and t1[0] >= -1 and t1[-1] <= n_tiles - 1
            for k in range(0, n_tiles + 1):
                want = next((p for p in range(limit) if t1[p] >= k), limit)
                assert L.eq_first(k, t, limit) == want, (t, n_tiles, k)


# ------------------------------------------------------------------------------------------ header == restatement
def _cases(sizes=SIZES):
    for w, h in sizes:
        for tiles in TILES:
            if tiles[0] > w or tiles[1] > h:
                continue
            yield w, h, tiles


@pytest.mark.parametrize("w,h", SIZES)
def test_header_equals_restatement(harness, w, h):
    n = 0
    for name, img in ER.structured_images(w, h).items():
        assert np.array_equal(harness.run(img, 1), ER.equalize_hist(img)), (name, "global")
        for _, _, tiles in _cases([(w, h)]):
            for clip in CLIPS:
                got, luts = harness.run(img, 2, tiles, clip, want_luts=True)
                assert np.array_equal(luts, ER.clahe_luts(img, tiles[0], tiles[1], clip)), (name, tiles, clip, "luts")
                assert np.array_equal(got, ER.clahe(img, tiles[0], tiles[1], clip)), (name, tiles, clip)
                n += 1
    assert n == len(ER.structured_images(w, h)) * len(TILES) * len(CLIPS)


@pytest.mark.parametrize("mutation", ER.MUTATIONS)
def test_the_set_sees_mutations(harness, mutation):
    """Each deliberate mistake in the restatement changes at least one output byte somewhere on the set (the small sizes of
    it are enough), so the comparison above would catch the same mistake in the header."""
    changed = 0
    for w, h, tiles in _cases(SIZES[:4]):
        for name, img in ER.structured_images(w, h).items():
            for clip in CLIPS:
                good = harness.run(img, 2, tiles, clip)
                bad = ER.clahe(img, tiles[0], tiles[1], clip, mutate=mutation)
                changed += int(not np.array_equal(good, bad))
            if mutation == "truncate":
                changed += int(not np.array_equal(harness.run(img, 1), ER.equalize_hist(img, mutate=mutation)))
    assert changed > 0


def test_cv2_cross_check():
    """Optional: OpenCV's own equalizeHist / CLAHE, where the module is installed (sizes the tiles divide and ragged sizes
    whose extended rows stay within 2 h - 2, where the contract claims parity)."""
    cv2 = pytest.importorskip("cv2")
    for w, h in [(64, 64), (188, 120), (67, 45)]:
        for name, img in ER.structured_images(w, h).items():
            assert np.array_equal(cv2.equalizeHist(img), ER.equalize_hist(img)), name
            for clip in (1.0, 3.0, 40.0):
                c = cv2.createCLAHE(clipLimit=clip, tileGridSize=(8, 8))
                assert np.array_equal(c.apply(img), ER.clahe(img, 8, 8, clip)), (name, clip)
