"""The image-mask contract ("Image masks") on the CPU: known answers of the numpy restatement
(tests/mask_reference.py), csrc/hip/fe_mask.h (the header the kernels and the C ABI run) compiled with g++ == the restatement,
bit for bit, the gate at the rounding edges of the pixel rule, and the deliberate mistakes of mask_reference.MUTATIONS, each of
which changes some expected output of these cases."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import detector_cases as DC
import detector_reference as DR
import mask_reference as MR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(17, 17), (31, 9), (32, 40), (33, 33), (65, 47), (188, 120)]       # w, h
DENSITIES = [0.5, 0.01, 0.99]                                               # share of masked-out pixels
MARGINS = [0, 1, 5, 64]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("fe_mask") / "libfe_mask_test.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-shared", "-fPIC", "-I", ROOT, "-o", so,
                           os.path.join(ROOT, "tests", "cpp", "fe_mask_test.cpp")])
    L = C.CDLL(so)
    L.fm_run.argtypes = [C.c_void_p, C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.fm_pixel_of.argtypes = [C.c_float]
    L.fm_lookup.argtypes = [C.c_void_p] + [C.c_int] * 4
    L.fm_gate_points.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 5
    L.fm_gate_points.restype = None

    class H:
        lib = L

        @staticmethod
        def run(mask, margin, pad=0):
            """(usable, words, unpacked) of the header for a mask whose rows lie `pad` bytes further apart than dense."""
            h, w = mask.shape
            src = np.full((h, w + pad), 0x5A, np.uint8)
            src[:, :w] = mask
            usable, words, unpacked = np.zeros((h, w), np.uint8), np.zeros((h, MR.pitch_words(w)), np.uint32), np.zeros((h, w), np.uint8)
            assert L.fm_run(src.ctypes.data, w + pad, w, h, margin, usable.ctypes.data, words.ctypes.data, unpacked.ctypes.data) == 0
            return usable, words, unpacked

        @staticmethod
        def gate(m0, m1, w, h, out0, out1, und0, und1, status):
            a = [np.array(x, np.float32).reshape(-1, 2) for x in (out0, out1, und0, und1)]
            st = np.array(status, np.uint8)
            L.fm_gate_points(None if m0 is None else m0.ctypes.data, None if m1 is None else m1.ctypes.data, w, h, len(st),
                             *[x.ctypes.data for x in a], st.ctypes.data)
            return (*a, st)
    return H


def random_mask(w, h, density, seed):
    """uint8 plane, `density` of its pixels 0, the others of any non-zero value."""
    rng = np.random.default_rng([w, h, int(density * 1000), seed])
    return np.where(rng.random((h, w)) < density, 0, rng.integers(1, 256, (h, w))).astype(np.uint8)


# ------------------------------------------------------------------------------------------ known answers
def test_single_zero_pixel():
    m = np.full((9, 11), 255, np.uint8)
    m[4, 6] = 0
    e0, e1 = MR.erode(m, 0), MR.erode(m, 1)
    assert e0.sum() == 9 * 11 - 1 and not e0[4, 6]
    assert e1.sum() == 9 * 11 - 9 and not e1[3:6, 5:8].any()
    assert MR.erode(m, 2).sum() == 9 * 11 - 25


def test_zero_pixel_at_a_corner():
    m = np.ones((9, 11), np.uint8)
    m[0, 0] = 0
    e = MR.erode(m, 2)
    assert not e[:3, :3].any() and e.sum() == 9 * 11 - 9          # the window is cut at the image, and the border masks nothing
    assert MR.erode(np.ones((9, 11), np.uint8), 64).all()


@pytest.mark.parametrize("w", [31, 32, 33, 65])
def test_padding_bits(w):
    words = MR.pack(np.ones((3, w), bool))
    assert words.shape == (3, (w + 31) // 32) and words.dtype == np.uint32
    full, rest = divmod(w, 32)
    assert np.all(words[:, :full] == 0xFFFFFFFF)
    if rest:
        assert np.all(words[:, full] == (1 << rest) - 1)
    one = np.zeros((3, w), bool)
    one[1, w - 1] = True
    assert MR.pack(one)[1, (w - 1) >> 5] == 1 << ((w - 1) & 31) and MR.pack(one).sum() == 1 << ((w - 1) & 31)
    assert MR.lookup(MR.pack(one), w, 3, w - 1, 1) and not MR.lookup(MR.pack(one), w, 3, w - 2, 1)
    assert MR.lookup(MR.pack(one), w, 3, w, 1) and MR.lookup(MR.pack(one), w, 3, -1, 1)          # outside: usable


def test_pixel_rule_known_answers(harness):
    below = np.nextafter(np.float32(7.5), np.float32(0))
    for v, want in [(7.5, 8), (below, 7), (0.0, 0), (0.49, 0), (187.0, 187), (187.4, 187), (8388607.0, 8388607)]:
        assert int(MR.pixel(np.float32(v))) == want == harness.lib.fm_pixel_of(float(np.float32(v)))
    # float32 addition: 0.49999997 + 0.5 rounds to 1.0f
    v = np.nextafter(np.float32(0.5), np.float32(0))
    assert int(MR.pixel(v)) == 1 == harness.lib.fm_pixel_of(float(v))


# ------------------------------------------------------------------------------------------ the header == the restatement
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_header_equals_restatement(harness, size):
    w, h = size
    assert harness.lib.fm_max_margin() == MR.MAX_MARGIN and harness.lib.fm_words_per_row(w) == MR.pitch_words(w)
    for density in DENSITIES:
        mask = random_mask(w, h, density, 1)
        for margin in MARGINS:
            want = MR.erode(mask, margin)
            words = MR.pack(want)
            for pad in (0, 5):
                usable, got_words, unpacked = harness.run(mask, margin, pad)
                assert np.array_equal(usable != 0, want), (size, density, margin, pad)
                assert np.array_equal(got_words, words)
                assert np.array_equal(unpacked, np.where(want, 255, 0))
            if margin == 0:
                yy, xx = np.mgrid[-1:h + 1, -1:w + 1]
                got = np.array([harness.lib.fm_lookup(words.ctypes.data, w, h, int(x), int(y)) for x, y in zip(xx.ravel(), yy.ravel())], bool)
                assert np.array_equal(got, MR.lookup(words, w, h, xx.ravel(), yy.ravel()))


# ------------------------------------------------------------------------------------------ the gate
W, H = 70, 40


def gate_points():
    """Synthetic track outputs around the edges of the pixel rule: for each status 0, 1, 3 a block of points whose out0 / out1 sit
    at x = k + 0.5 exactly, just below it, at 0 and at W - 1 (y likewise), the other coordinate mid-pixel."""
    below = lambda k: np.nextafter(np.float32(k + 0.5), np.float32(0))
    xs = [0.0, 0.25, 0.5, below(0), 31.5, below(31), 32.5, below(32), 32.0, W - 1.0, W - 1.25, 10.0]
    ys = [0.0, 0.5, below(0), 20.5, below(20), H - 1.0, 7.0]
    pts = np.array([(x, y) for x in xs for y in ys], np.float32)
    n = len(pts)
    out0 = np.concatenate([pts] * 3)
    out1 = np.concatenate([pts[::-1]] * 3)           # another point of the same set under cam1
    status = np.repeat(np.array([0, 1, 3], np.uint8), n)
    rng = np.random.default_rng(11)
    und0, und1 = rng.standard_normal((3 * n, 2)).astype(np.float32), rng.standard_normal((3 * n, 2)).astype(np.float32)
    return out0, out1, und0, und1, status


def gate_masks():
    """A cam0 and a cam1 plane whose zero pixels sit beside the points' pixels: single pixels, columns 31 / 32, row 20, the corners."""
    m0, m1 = np.ones((H, W), bool), np.ones((H, W), bool)
    m0[:, 32] = False; m0[21, :] = False; m0[0, 0] = False; m0[H - 1, W - 1] = False; m0[7, 10] = False
    m1[:, 31] = False; m1[20, :] = False; m1[1, 1] = False; m1[0, W - 1] = False; m1[7, 1] = False
    return MR.pack(m0), MR.pack(m1)


@pytest.mark.parametrize("which", ["both", "mask0", "mask1", "neither"])
def test_gate_header_equals_restatement(harness, which):
    m0, m1 = gate_masks()
    m0, m1 = (m0 if which in ("both", "mask0") else None), (m1 if which in ("both", "mask1") else None)
    pts = gate_points()
    want = MR.gate(m0, m1, W, H, *pts)
    got = harness.gate(m0, m1, W, H, *pts)
    for a, b in zip(want, got):
        assert a.tobytes() == b.tobytes()
    out0, out1, und0, und1, status = pts
    assert np.array_equal(want[0], out0)                                   # out0 is always kept
    lost = (status != 0) & (want[4] == 0)
    unmatched = (status == 3) & (want[4] == 1)
    if which == "neither":
        assert not lost.any() and not unmatched.any()
    else:
        assert (lost.any() or which == "mask1") and (unmatched.any() or which == "mask0")
    assert np.all(want[1][lost] == 0) and np.all(want[2][lost] == 0) and np.all(want[3][lost] == 0)
    keep = ~lost
    assert np.array_equal(want[1][keep], out1[keep]) and np.array_equal(want[2][keep], und0[keep]) and np.array_equal(want[3][keep], und1[keep])
    assert np.array_equal(want[4][status == 0], status[status == 0])


# ------------------------------------------------------------------------------------------ masked cell maxima
def test_masked_maxima_known_answers():
    case = DC.like16("m", "random", 72, 48, seed=3)
    img = DC.image(case.kind, case.w, case.h, case.seed)
    score = DR.score_map(img)
    plain = DR.reduce_cells(score, case.rows, case.cols, case.cw, case.ch)
    assert np.array_equal(MR.masked_cell_maxima(score, np.ones_like(score, bool), case.rows, case.cols, case.cw, case.ch), plain)
    assert not MR.masked_cell_maxima(score, np.zeros_like(score, bool), case.rows, case.cols, case.cw, case.ch)["has"].any()
    u = np.ones_like(score, bool)
    u[plain["y"][plain["has"]], plain["x"][plain["has"]]] = False
    nxt = MR.masked_cell_maxima(score, u, case.rows, case.cols, case.cw, case.ch)
    both = plain["has"] & nxt["has"]
    assert both.any() and np.all(nxt["score"][both] <= plain["score"][both])
    assert not np.any((nxt["x"][both] == plain["x"][both]) & (nxt["y"][both] == plain["y"][both]))


# ------------------------------------------------------------------------------------------ the mistakes would be seen
def _expected_outputs(mutate=None):
    """Everything the cases above expect, under one mistake."""
    out = []
    for (w, h) in [(33, 33), (65, 47)]:
        mask = random_mask(w, h, 0.01, 1)
        for margin in (0, 1, 5):
            out.append(MR.pack(MR.erode(mask, margin, mutate), mutate).tobytes())
    m0, m1 = gate_masks()
    for a in MR.gate(m0, m1, W, H, *gate_points(), mutate=mutate):
        out.append(a.tobytes())
    return out


@pytest.mark.parametrize("mutate", MR.MUTATIONS)
def test_every_mistake_changes_an_expected_output(mutate):
    want, got = _expected_outputs(), _expected_outputs(mutate)
    changed = [k for k, (a, b) in enumerate(zip(want, got)) if a != b]
    assert changed, mutate
    if mutate in ("margin_minus_one", "margin_plus_one", "msb_first", "outside_masked"):
        assert all(k < 6 for k in changed)          # the planes; the gate reads the same planes and is untouched
    else:
        assert all(k >= 6 for k in changed)         # the gate's outputs
