"""The input-pixel-format contract ("Input pixel formats") on the CPU: known answers of the numpy restatement
(tests/pixel_format_reference.py), and csrc/hip/fe_pixfmt.h (the header the kernel runs) compiled with g++ == the restatement,
byte for byte, over a set of images that three deliberate mistakes in the restatement each change."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import pixel_format_reference as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(16, 16), (40, 24), (67, 45), (188, 120), (333, 251), (752, 480)]       # w, h
SHIFTS = [0, 2, 4, 8]
COLOUR = ["rgb8", "bgr8", "rgba8", "bgra8"]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("fe_pixfmt") / "libfe_pixfmt_test.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-shared", "-fPIC", "-I", ROOT, "-o", so,
                           os.path.join(ROOT, "tests", "cpp", "fe_pixfmt_test.cpp")])
    L = C.CDLL(so)
    L.px_run.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_longlong, C.c_void_p, C.c_int, C.c_int]

    class H:
        lib = L

        @staticmethod
        def run(raw, fmt, shift=0, pad=0):
            """The header's conversion of a raw image, its rows `pad` bytes further apart than dense."""
            name = PR.name_of(fmt)
            h, w = raw.shape[:2]
            src = PR.raw_bytes(raw, name, pad)
            assert src.shape == (h, w * PR.BPP[name] + pad)
            dst = np.zeros((h, w), np.uint8)
            assert L.px_run(PR.FORMATS[name], shift, src.ctypes.data, src.shape[1], dst.ctypes.data, w, h) == 0
            return dst
    return H


def both(harness, raw, fmt, shift=0):
    """The restatement's output, after checking that the header's is the same (dense and pitched)."""
    a = PR.convert(raw, fmt, shift)
    assert np.array_equal(a, harness.run(raw, fmt, shift)) and np.array_equal(a, harness.run(raw, fmt, shift, pad=6))
    return a


def test_px_job_layout_matches_the_header(harness):
    out = (C.c_int * 16)()
    n = harness.lib.px_job_layout(out, 16)
    assert n == len(PR.PxJob._fields_) + 1
    assert list(out[:n]) == [C.sizeof(PR.PxJob)] + [getattr(PR.PxJob, name).offset for name, _ in PR.PxJob._fields_]


# ------------------------------------------------------------------------------------------ known answers
def test_format_table(harness):
    assert [harness.lib.px_bytes_per_pixel(v) for v in range(10)] == [PR.BPP[PR.NAMES[v]] for v in range(10)] == [1, 2, 3, 3, 4, 4, 1, 1, 1, 1]
    assert harness.lib.px_bytes_per_pixel(10) == 0 and harness.lib.px_bytes_per_pixel(-1) == 0


def test_luma_known_answers(harness):
    L = harness.lib
    for rgb, want in {(255, 0, 0): 76, (0, 255, 0): 150, (0, 0, 255): 29}.items():
        assert L.px_luma_of(*rgb) == want == int(PR.luma(*rgb))
    assert 76 + 150 + 29 == 255
    v = np.arange(256)
    assert np.array_equal(PR.luma(v, v, v), v)
    assert [L.px_luma_of(int(k), int(k), int(k)) for k in v] == list(v)


def test_colour_orders_agree_on_permuted_data(harness):
    """BGR / RGBA / BGRA give what RGB gives on the permuted data, whatever the fourth byte holds."""
    rng = np.random.default_rng(5)
    rgb = rng.integers(0, 256, (45, 67, 3)).astype(np.uint8)
    want = both(harness, rgb, "rgb8")
    assert np.array_equal(both(harness, rgb[..., ::-1], "bgr8"), want)
    for alpha in (0, 255, None):
        a = rng.integers(0, 256, (45, 67, 1)).astype(np.uint8) if alpha is None else np.full((45, 67, 1), alpha, np.uint8)
        assert np.array_equal(both(harness, np.concatenate([rgb, a], axis=2), "rgba8"), want)
        assert np.array_equal(both(harness, np.concatenate([rgb[..., ::-1], a], axis=2), "bgra8"), want)


def test_gray16_known_answers(harness):
    L = harness.lib
    for v, shift, want in [(0x0FFF, 4, 255), (0x1000, 4, 255), (256, 0, 255), (0xFF00, 8, 255), (255, 0, 255), (0xFFFF, 0, 255), (0xFFFF, 8, 255), (0x0FF0, 4, 255),
                           (0x0FEF, 4, 254), (3, 2, 0), (4, 2, 1)]:
        assert L.px_gray16_of(v, shift) == want == int(PR.gray16(v, shift)), (v, shift)
    g = np.arange(256, dtype=np.uint16).reshape(16, 16)
    for n in range(16):
        assert np.array_equal(both(harness, (g << 4) | n, "gray16", 4), g.astype(np.uint8))


def _mosaic(fmt, w, h, a, b, c):
    """The mosaic of the pattern in which every red site holds a, every green site b, every blue site c."""
    letters = fmt[len("bayer_"):len("bayer_") + 4].upper()
    yy, xx = np.mgrid[0:h, 0:w]
    site = np.array(list(letters))[(yy & 1) * 2 + (xx & 1)]
    return np.select([site == "R", site == "G"], [a, b], c).astype(np.uint8)


@pytest.mark.parametrize("fmt", PR.BAYER)
def test_bayer_flat_colour_gives_its_luma_everywhere(harness, fmt):
    """R = a, G = b, B = c on every site: luma(a, b, c) at EVERY pixel, borders and corners included (REFLECT_101 keeps the site
    colour and the rounded means of equal values are exact), for even and odd sizes."""
    for w, h in [(16, 16), (17, 16), (16, 17), (67, 45), (2, 2), (3, 2), (2, 3)]:
        for a, b, c in [(255, 0, 0), (0, 255, 0), (0, 0, 255), (200, 90, 31), (255, 255, 255), (1, 2, 3)]:
            out = both(harness, _mosaic(fmt, w, h, a, b, c), fmt)
            assert (out == int(PR.luma(a, b, c))).all(), (w, h, a, b, c)


def test_bayer_patterns_agree_on_a_shifted_mosaic(harness):
    """A mosaic cut one column, one row, or both further in is the mosaic of another pattern: away from the border the four
    patterns give the same pixels."""
    rng = np.random.default_rng(9)
    big = rng.integers(0, 256, (47, 69)).astype(np.uint8)
    h, w = 45, 67
    base = both(harness, big[:h, :w], "bayer_rggb8")
    for fmt, (dx, dy) in {"bayer_grbg8": (1, 0), "bayer_gbrg8": (0, 1), "bayer_bggr8": (1, 1)}.items():
        out = both(harness, big[dy:dy + h, dx:dx + w], fmt)
        # pixel (x, y) of the shifted cut is pixel (x + dx, y + dy) of the base
        assert np.array_equal(out[1:h - 2, 1:w - 2], base[1 + dy:h - 2 + dy, 1 + dx:w - 2 + dx]), fmt
    assert not np.array_equal(both(harness, big[:h, :w], "bayer_bggr8"), base)


def test_reflect(harness):
    L = harness.lib
    assert [L.px_reflect_of(i, 8) for i in (-1, 0, 7, 8)] == [1, 0, 7, 6]
    assert [L.px_reflect_of(i, 2) for i in (-1, 0, 1, 2)] == [1, 0, 1, 0]


# ------------------------------------------------------------------------------------------ header == restatement
def _cases():
    for name in PR.FORMATS:
        for shift in (SHIFTS if name == "gray16" else [0]):
            yield name, shift


@pytest.mark.parametrize("w,h", SIZES)
def test_header_equals_restatement(harness, w, h):
    n = 0
    for name, shift in _cases():
        for kind, raw in PR.raw_images(w, h, name, seed=1, shift=shift).items():
            want = PR.convert(raw, name, shift)
            for pad in (0, 6):
                assert np.array_equal(harness.run(raw, name, shift, pad), want), (name, shift, kind, pad)
                n += 1
    assert n == (len(PR.FORMATS) - 1 + len(SHIFTS)) * 8 * 2


@pytest.mark.parametrize("mutation", PR.MUTATIONS)
def test_the_set_sees_mutations(harness, mutation):
    """Each deliberate mistake in the restatement changes at least one output byte somewhere on the set (the small sizes of
    it are enough), so the comparison above would catch the same mistake in the header."""
    changed = 0
    for w, h in SIZES[:4]:
        for name, shift in _cases():
            for raw in PR.raw_images(w, h, name, seed=1, shift=shift).values():
                changed += int(not np.array_equal(harness.run(raw, name, shift), PR.convert(raw, name, shift, mutate=mutation)))
    assert changed > 0


def test_cv2_cross_check():
    """Optional: OpenCV's own 8-bit RGB2GRAY, where the module is installed."""
    cv2 = pytest.importorskip("cv2")
    raw = PR.raw_images(188, 120, "rgb8")["random"]
    assert np.array_equal(cv2.cvtColor(raw, cv2.COLOR_RGB2GRAY), PR.convert(raw, "rgb8"))
