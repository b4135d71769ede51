"""The descriptor contract ("Descriptors") on the CPU: the facts of the generated pattern, known answers of the
numpy restatement (tests/brief_reference.py), csrc/hip/fe_brief.h (the header the kernel and the C ABI run) compiled with g++ ==
the restatement, bit for bit, on the sizes, image kinds and points of tests/brief_cases.py, the deliberate mistakes of
brief_reference.MUTATIONS, each of which changes some expected output of these cases, and the property that makes the
descriptor worth having: a point is much closer to itself in a moved, noisy view than to another point."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import brief_cases as BC
import brief_reference as BR
import lk_cases as LK

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("fe_brief") / "libfe_brief_test.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-shared", "-fPIC", "-I", ROOT, "-o", so,
                           os.path.join(ROOT, "tests", "cpp", "fe_brief_test.cpp")])
    L = C.CDLL(so)
    L.fb_pattern.argtypes = [C.c_void_p]
    L.fb_valid_of.argtypes = [C.c_float, C.c_float, C.c_int, C.c_int]
    L.fb_centre_of.argtypes = [C.c_float]
    L.fb_describe.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_longlong, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]

    class H:
        lib = L

        @staticmethod
        def describe(img, pts, pitch=None):
            h, w = img.shape
            buf = np.ascontiguousarray(img) if pitch is None else BC.padded(img, pitch)
            pts = np.ascontiguousarray(pts, dtype=np.float32).reshape(-1, 2)
            desc, valid = np.full((len(pts), 32), 0xEE, np.uint8), np.full(len(pts), 0xEE, np.uint8)
            assert L.fb_describe(buf.ctypes.data, w, h, buf.shape[1], pts.ctypes.data, len(pts), desc.ctypes.data, valid.ctypes.data) == 0
            return desc, valid
    return H


def bits_of(desc):
    """(n, 256) 0 / 1: bit t of the contract."""
    return np.unpackbits(desc, axis=1, bitorder="little")


# ------------------------------------------------------------------------------------------ the pattern
def test_pattern_facts():
    assert BR.DRAWS == 1028                                        # 257 tests drawn: one compared a sum with itself
    assert BR.PATTERN.shape == (256, 4)
    assert len({tuple(t) for t in BR.PATTERN.tolist()}) == 256
    assert BR.PATTERN.min() == -12 and BR.PATTERN.max() == 12
    assert BR.PATTERN[:3].tolist() == [[3, 0, 5, -2], [-2, 9, -3, -7], [-2, 5, 9, 2]]
    assert not ((BR.PATTERN[:, 0] == BR.PATTERN[:, 2]) & (BR.PATTERN[:, 1] == BR.PATTERN[:, 3])).any()


def test_header_pattern_is_the_generated_one(harness):
    out = np.zeros(1024, np.int8)
    assert harness.lib.fb_pattern(out.ctypes.data) == BR.DRAWS
    assert np.array_equal(out.reshape(256, 4), BR.PATTERN)


def test_abi_pattern_is_the_generated_one():
    """mskf_fe_descriptor_pattern makes no device call: it runs where there is no GPU."""
    from msckf_stereo_c_amd import build
    L = C.CDLL(build.build_hip())
    out = np.full(1024, 99, np.int8)
    L.mskf_fe_descriptor_pattern.argtypes = [C.c_void_p]
    L.mskf_fe_descriptor_pattern.restype = None
    L.mskf_fe_descriptor_pattern(out.ctypes.data)
    assert np.array_equal(out.reshape(256, 4), BR.PATTERN)


# ------------------------------------------------------------------------------------------ known answers
@pytest.mark.parametrize("level", [131, 255, 0])
def test_flat_image_gives_zeros(level):
    """Strictness: equal sums set no bit; 255 everywhere: a box sum of 6375 must not be kept in 8 bits."""
    img = np.full((40, 50), level, np.uint8)
    desc, valid = BR.describe(img, [[25, 20], [0, 0], [49, 39], [3.3, 38.6]])
    assert valid.tolist() == [1, 1, 1, 1] and not desc.any()
    assert BR.box_sums(img).max() == 25 * level


def test_ramps():
    yy, xx = np.mgrid[0:60, 0:60]
    centre = [[30, 30], [29.6, 30.4]]
    d, v = BR.describe((4 * xx).astype(np.uint8), centre)                      # 4 * (30 + 14) < 256: no wrap, no clamp
    assert v.all() and np.array_equal(bits_of(d), np.tile(BR.PATTERN[:, 0] < BR.PATTERN[:, 2], (2, 1)))
    d, v = BR.describe((4 * yy).astype(np.uint8), centre)
    assert v.all() and np.array_equal(bits_of(d), np.tile(BR.PATTERN[:, 1] < BR.PATTERN[:, 3], (2, 1)))


def test_one_pixel_image():
    desc, valid = BR.describe(np.array([[77]], np.uint8), [[0, 0], [-0.5, 0.25]])
    assert valid.tolist() == [1, 1] and not desc.any()             # everything clamps to the one pixel


def test_validity_edges_known():
    f = np.float32
    for w, h in [(1, 1), (64, 48)]:
        def valid_x(x):
            return bool(BR.valid_and_centre([[x, 0.0]], w, h)[0][0])
        assert valid_x(-0.5)
        assert not valid_x(-0.50000006)
        assert not valid_x(w - 0.5)
        assert valid_x(np.nextafter(f(w - 0.5), f(-np.inf))) == (w > 1)        # (0.49999997 + 0.5 rounds to 1)
        assert not valid_x(w - 1 + 0.5)
        for x in (np.nan, np.inf, -np.inf, 1e30, -1e30):
            assert not valid_x(x)
    # one pixel wide: W - 0.50000006 is a float32 of its own, and valid; k + 0.49999997 rounds up to W
    assert bool(BR.valid_and_centre([[1 - 0.50000006, 0.0]], 1, 1)[0][0])
    assert not bool(BR.valid_and_centre([[0.49999997, 0.0]], 1, 1)[0][0])
    # k + 0.49999997 + 0.5 rounds to k + 1 in float32: the centre is the next pixel; k + 0.5 likewise
    v, cx, cy = BR.valid_and_centre([[0.49999997, 5.49999997], [7.5, 7.25], [-0.5, 47.4]], 64, 48)
    assert v.all() and cx.tolist() == [1, 8, 0] and cy.tolist() == [6, 7, 47]       # (5.49999997 is 5.5 in float32)
    # NaN on one axis only, and on the other
    v, _, _ = BR.valid_and_centre([[np.nan, 3], [3, np.nan], [3, 3]], 64, 48)
    assert v.tolist() == [False, False, True]


def test_invalid_point_gives_zeros():
    img = BC.image("random", 64, 64)
    desc, valid = BR.describe(img, [[-1, 5], [5, 64], [np.nan, 5], [30, 30]])
    assert valid.tolist() == [0, 0, 0, 1] and not desc[:3].any() and desc[3].any()


# ------------------------------------------------------------------------------------------ the header against the restatement
@pytest.mark.parametrize("kind", BC.KINDS)
@pytest.mark.parametrize("size", BC.SIZES, ids=lambda s: "%dx%d" % s)
def test_header_equals_restatement(harness, size, kind):
    w, h = size
    img, pts = BC.image(kind, w, h), BC.points(w, h)
    want_d, want_v = BR.describe(img, pts)
    got_d, got_v = harness.describe(img, pts, BC.PITCH.get(size))
    assert np.array_equal(got_v, want_v)
    assert np.array_equal(got_d, want_d)
    assert 0 < want_v.sum() < len(pts)                             # both kinds of point are there


def test_header_validity_and_centre(harness):
    for w, h in BC.SIZES:
        pts = BC.validity_edges(w, h)
        v, cx, cy = BR.valid_and_centre(pts, w, h)
        for p, vi, x, y in zip(pts, v, cx, cy):
            assert harness.lib.fb_valid_of(p[0], p[1], w, h) == int(vi), (w, h, p)
            if vi:
                assert (harness.lib.fb_centre_of(p[0]), harness.lib.fb_centre_of(p[1])) == (x, y), (w, h, p)


def test_cases_are_alive():
    """The cases set both values of many bits, reach every clamped side, and hold every distance 0 .. 14 from every side."""
    for kind in BC.KINDS:
        img = BC.image(kind, 129, 71)
        b = bits_of(BR.describe(img, BC.lattice(129, 71))[0])
        if kind != "checker1":                                     # (every 5 x 5 box of the period-2 checkerboard holds 12 or 13 white pixels)
            assert ((b.mean(axis=0) > 0.05) & (b.mean(axis=0) < 0.95)).sum() > 200, kind
    for w, h in BC.SIZES:
        c = BC.border_centres(w, h)
        for d in range(min(BC.FOOT, w - 1) + 1):
            assert (c[:, 0] == d).any() and (c[:, 0] == w - 1 - d).any()
        for d in range(min(BC.FOOT, h - 1) + 1):
            assert (c[:, 1] == d).any() and (c[:, 1] == h - 1 - d).any()
        for corner in [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1)]:
            assert (c == np.array(corner, np.float32)).all(axis=1).any()


# ------------------------------------------------------------------------------------------ planted mistakes
def _mutation_outputs(mutation):
    """Does the mistake change the expected output of a case?  The first that does."""
    flat = np.full((40, 40), 90, np.uint8)
    yy, xx = np.mgrid[0:40, 0:40]
    extra = [("flat", flat, np.array([[20, 20]], np.float32)), ("ramp", (3 * xx + 2 * yy).astype(np.uint8), np.array([[20, 20]], np.float32))]
    cases = extra + [("%s %dx%d" % (kind, w, h), BC.image(kind, w, h), BC.points(w, h)) for (w, h) in [(30, 31), (64, 64)] for kind in BC.KINDS]
    for name, img, pts in cases:
        d0, v0 = BR.describe(img, pts)
        d1, v1 = BR.describe(img, pts, mutation=mutation)
        if not (np.array_equal(d0, d1) and np.array_equal(v0, v1)):
            return name
    return None


@pytest.mark.parametrize("mutation", BR.MUTATIONS)
def test_every_planted_mistake_shows(mutation):
    assert _mutation_outputs(mutation) is not None


def test_planted_mistakes_are_the_listed_ones():
    assert set(BR.MUTATIONS) == {"le_for_lt", "box_radius_1", "swap_ax_ay", "zero_padding", "truncate_without_half", "bit_order_reversed", "swap_t_t64"}
    flat = np.full((40, 40), 90, np.uint8)
    assert BR.describe(flat, [[20, 20]], mutation="le_for_lt")[0].min() == 255          # the flat image is what catches it
    assert _mutation_outputs(None) is None                                               # no mistake: nothing differs


# ------------------------------------------------------------------------------------------ worth having
WORTH = {}          # canvas -> (median distance to itself in the other view, median distance between different points)


@pytest.mark.parametrize("name", ["smooth", "blocks8", "edges"])
def test_descriptor_recognises_a_point(name):
    """160 x 120 views of one canvas, the second moved by (3, -2) with uniform noise of +-4 grey levels; a 9 px lattice 20 px
    inside.  The median Hamming distance of a point to itself in the other view is at most a third of the median distance
    between different points.  (A CPU property of the contract: the device computes the same bits.)"""
    w, h, seed = 160, 120, 7
    canvas = {"smooth": lambda: LK.smooth_canvas(w, h, seed), "blocks8": lambda: LK.block_canvas(w, h, 8, seed), "edges": lambda: LK.edge_canvas(w, h, seed)}[name]()
    A = LK.crop(canvas, w, h)
    noise = np.random.default_rng(seed).integers(-4, 5, (h, w))
    B = (LK.crop(canvas, w, h, 3, -2).astype(np.int64) + noise).clip(0, 255).astype(np.uint8)
    pts = np.array([(x, y) for y in range(20, h - 20, 9) for x in range(20, w - 20, 9)], np.float32)
    dA, vA = BR.describe(A, pts)
    dB, vB = BR.describe(B, pts + np.array([3, -2], np.float32))          # a feature at p in A is at p + (3, -2) in B
    assert vA.all() and vB.all()
    same = BR.hamming(dA, dB)
    cross = BR.hamming(dA[:, None, :], dB[None, :, :])
    other = cross[~np.eye(len(pts), dtype=bool)]
    m_same, m_other = float(np.median(same)), float(np.median(other))
    WORTH[name] = (m_same, m_other)
    print("descriptor medians %s: same point %.1f, different points %.1f" % (name, m_same, m_other))
    assert m_same <= m_other / 3.0
