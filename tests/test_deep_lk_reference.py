"""The numpy restatement of the L-level LK (tests/deep_lk_reference.py) pinned on the CPU, before the GPU tests compare the device
with it (tests/test_gpu_lk_levels.py): at L = 4 it is the oracle, at L = 8 two chained oracle runs, its capture range grows with the
depth and too deep is harmful, three planted mistakes each change a result; the validity rule of csrc/hip/fe_deep.h through a g++
harness; the app's yaml key."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import deep_lk_reference as D
import lk_cases as LC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = (129, 71)                 # the one small size of the L = 4 pin (odd sides, level 3 is 17 x 9)
RANGE_SIZE, RANGE_SHIFT = (640, 512), 52
BIG_SIZE, BIG_SHIFT = (2048, 1920), 24


# ------------------------------------------------------------------------------------------ L = 4: the oracle
@pytest.mark.parametrize("set_name", ["displaced", "border", "saturated"])
def test_four_levels_are_the_oracle(oracle, set_name):
    """Bits and statuses of oracle_py.lk_track on every case of the set (the border lattice: every third point)."""
    w, h = SMALL
    n_lost = n_pts = 0
    for c in LC.cases(set_name, w, h, oracle):
        pts = c["pts"][::3] if set_name == "border" else c["pts"][::2]
        guess = LC.hpred_guess(c["H"], pts)
        ref_b, ref_st = oracle.lk_track(c["A"], c["B"], pts, guess)
        b, st = D.lk_track(c["A"], c["B"], pts, guess, 4)
        assert np.array_equal(st, ref_st), c["name"]
        assert LC.same(b, ref_b), c["name"]               # (the oracle returns the position whatever the status: all points)
        n_lost += int((ref_st == 0).sum())
        n_pts += len(pts)
    assert n_pts > 200 and 0 < n_lost < n_pts


def test_restated_stereo_match_is_the_oracle_at_four_levels(oracle):
    from msckf_stereo_c_amd.ctypes_types import default_fe_cfg
    w, h = 376, 240
    c = LC.cases("sizes", w, h, oracle)[0]
    calib, fe = oracle.euroc_calib(w, h), default_fe_cfg()
    pts = c["pts"][::5]
    ref_c1, ref_in = oracle.stereo_match(calib, fe, c["B"], c["B1"], pts)
    c1, inl = D.stereo_match(oracle, calib, fe, c["B"], c["B1"], pts, 4)
    assert LC.same(c1, ref_c1) and np.array_equal(inl, ref_in) and 10 < ref_in.sum()
    # ... and where the epipolar gate refuses: cam1 moved three rows down
    B1 = LC.shifted_replicate(c["B1"], 0, 3)
    ref_c1, ref_in = oracle.stereo_match(calib, fe, c["B"], B1, pts)
    c1, inl = D.stereo_match(oracle, calib, fe, c["B"], B1, pts, 4)
    assert LC.same(c1, ref_c1) and np.array_equal(inl, ref_in)


# ------------------------------------------------------------------------------------------ L = 8: two chained oracle runs
def test_eight_levels_are_two_chained_oracle_runs(oracle):
    """lk_track on the level-4 images with points and guess divided by 16, then lk_track on level 0 with that result times 16 as
    the guess: exact, since every scaling is a power of two and the oracle returns the position whatever the status."""
    w, h = RANGE_SIZE
    for shift in (8, 60):
        A, B, pts = D.scene(w, h, shift)
        guess = (pts + np.array([3.0, -2.0], np.float32)).astype(np.float32)
        pa, pb = D.pyramid(A, 5), D.pyramid(B, 5)
        top, _ = oracle.lk_track(pa[4], pb[4], pts / np.float32(16), guess / np.float32(16))
        ref_b, ref_st = oracle.lk_track(A, B, pts, top * np.float32(16))
        b, st = D.lk_track(A, B, pts, guess, 8)
        assert np.array_equal(st, ref_st) and LC.same(b, ref_b), shift
        assert len(pts) >= 30


# ------------------------------------------------------------------------------------------ capture range
_COUNTS = {}


def range_counts():
    """{(size, shift, L): bool per point} on the capture-range scenes; the point set of a size is the same for every shift."""
    if not _COUNTS:
        for (w, h), shifts, depths in ((RANGE_SIZE, (8, RANGE_SHIFT), (4, 5, 6)), (BIG_SIZE, (8, BIG_SHIFT), (4, 8))):
            for shift in shifts:
                A, B, pts = D.scene(w, h, shift)
                for L in depths:
                    if shift == 8 and L != 4:
                        continue
                    b, st = D.lk_track(A, B, pts, pts, L)
                    _COUNTS[((w, h), shift, L)] = D.tracked(b, st, pts, shift)
    return _COUNTS


def test_depth_extends_the_capture_range(oracle):
    """640 x 512, seed 7, the points a shift of 8 px tracks at four levels (32 of 36): at 52 px four levels keep 12 of them
    (fewer than half), five 24, six 30 (at least 90 %).  At the 60 px the issue measured the chained approximation at, the
    restatement gives 7 / 11 / 28 of 32: 87.5 % at six levels, so the shift that separates the two is 52 px."""
    T = range_counts()
    base = T[(RANGE_SIZE, 8, 4)]
    n = int(base.sum())
    got = {L: int((T[(RANGE_SIZE, RANGE_SHIFT, L)] & base).sum()) for L in (4, 5, 6)}
    print("capture range %dx%d shift %d: base %d of %d, L=4/5/6 -> %s" % (RANGE_SIZE + (RANGE_SHIFT, n, len(base), got)))
    assert n >= 30
    assert 2 * got[4] < n
    assert 10 * got[6] >= 9 * n
    assert got[4] <= got[5] <= got[6]


def test_too_deep_is_harmful(oracle):
    """2048 x 1920 at 24 px: eight levels track fewer points than four (25 against 44 of the 44 that 8 px tracks): the top
    levels hold no structure and send the guess astray.  The reason the depth is a per-stream choice."""
    T = range_counts()
    base = T[(BIG_SIZE, 8, 4)]
    n4, n8 = int((T[(BIG_SIZE, BIG_SHIFT, 4)] & base).sum()), int((T[(BIG_SIZE, BIG_SHIFT, 8)] & base).sum())
    print("too deep %dx%d shift %d: base %d, L=4 %d, L=8 %d" % (BIG_SIZE + (BIG_SHIFT, int(base.sum()), n4, n8)))
    assert base.sum() >= 40 and n8 < n4


# ------------------------------------------------------------------------------------------ planted mistakes
@pytest.mark.parametrize("mutate", D.MUTATIONS)
def test_a_planted_mistake_changes_a_result(oracle, mutate):
    w, h = RANGE_SIZE
    A, B, pts = D.scene(w, h, RANGE_SHIFT)
    if mutate == "status_from_top":
        # 2 x 2 px checks: the [1 4 6 4 1] filter has a zero at their frequency one level up, so every level from 2 on is flat
        # and fails its minEig test, while level 0 tracks: lost only with the mistake
        yy, xx = np.mgrid[0:h, 0:w]
        A = B = np.ascontiguousarray((((xx // 2 + yy // 2) % 2) * 255).astype(np.uint8))
        pts = np.array([[100.25, 90.5], [300.0, 200.0], [511.5, 333.25]], np.float32)
        assert (D.lk_track(A, B, pts, pts, 6)[1] == 1).all()
    good_b, good_st = D.lk_track(A, B, pts, pts, 6)
    bad_b, bad_st = D.lk_track(A, B, pts, pts, 6, mutate)
    assert not (LC.same(good_b, bad_b) and np.array_equal(good_st, bad_st))
    assert mutate in D.MUTATIONS and len(D.MUTATIONS) == 3


# ------------------------------------------------------------------------------------------ fe_deep.h through g++
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("fe_deep") / "libfe_deep_test.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-shared", "-fPIC", "-I", ROOT, "-o", so,
                           os.path.join(ROOT, "tests", "cpp", "fe_deep_test.cpp")])
    L = C.CDLL(so)
    L.fd_pyr_down.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    L.fd_pyr_down.restype = None
    return L


def test_validity_rule_of_the_header(harness):
    assert harness.fd_limits() == 4 | (8 << 8) | (15 << 16)
    for (w, h), most in (((752, 480), 6), ((3840, 2160), 8), ((239, 120), 4), ((240, 120), 4), ((240, 240), 5), ((512, 480), 6), ((517, 483), 6),
                         ((188, 120), 4), ((1280, 720), 6), ((1920, 1080), 7), ((1920, 1920), 8), ((64, 64), 4)):
        assert harness.fd_max_levels_of(w, h) == most == D.max_levels(w, h), (w, h)
        for L in range(0, 12):
            want = 1 if L < 4 or L > 8 else (2 if L > most else 0)
            assert harness.fd_validate_of(w, h, L) == want, (w, h, L)
    for n in (15, 16, 17, 239, 240, 517, 3840):
        for l in range(8):
            assert harness.fd_side_of(n, l) == D.level_sizes(n, n, 8)[l][0]
    rng = np.random.default_rng(5)
    for _ in range(200):                                   # the restated rule and the header agree everywhere
        w, h = int(rng.integers(16, 4200)), int(rng.integers(16, 4200))
        assert harness.fd_max_levels_of(w, h) == D.max_levels(w, h)


def test_pyr_down_of_the_header_is_the_oracle(harness, oracle):
    """Odd and even sides down to a 15-pixel level, and an image of extremes (the rounding at 255)."""
    rng = np.random.default_rng(11)
    for (w, h) in ((65, 61), (64, 60), (33, 31), (30, 29), (17, 16), (15, 15), (3, 3)):
        for img in (rng.integers(0, 256, (h, w), dtype=np.uint8), (rng.integers(0, 2, (h, w), dtype=np.uint8) * 255)):
            ref = oracle.pyr_down(img)
            out = np.zeros_like(ref)
            harness.fd_pyr_down(img.ctypes.data, w, h, out.ctypes.data)
            assert np.array_equal(out, ref), (w, h)


def test_device_records_are_laid_out_as_documented(harness):
    out = (C.c_int * 16)()
    n = harness.fd_dev_layout(out, 16)
    # PyrDeepDev: four pointers, four widths, four heights; FeDeepDev: three of them, levels, pad; DeepPyrJob: src, dst[4], w, h, levels, pad
    assert list(out[:n]) == [3 * 64 + 8, 64, 32, 48, 64, 128, 192, 56, 8, 40, 48]


# ------------------------------------------------------------------------------------------ the YAML key
def test_lk_pyramid_levels_yaml_key(tmp_path):
    from msckf_stereo_c_amd import build
    build.build_all()
    L = C.CDLL(os.path.join(ROOT, "msckf_stereo_c_amd", "_build", "libmskf_host.so"))
    L.mskfh_load_lk_levels.argtypes = [C.c_char_p, C.c_int, C.c_int, C.POINTER(C.c_int)]
    L.mskfh_load_lk_levels_error.restype = C.c_char_p

    def load(path, w=752, h=480):
        v = C.c_int(-1)
        rc = L.mskfh_load_lk_levels(str(path).encode(), w, h, C.byref(v))
        return rc, v.value
    stock = os.path.join(ROOT, "config", "app_imgproc.yaml")
    text = open(stock).read()
    assert "pyramid_levels" in text and "lk_pyramid_levels" not in text
    assert load(stock) == (0, 4)                                        # absent means 4; the reference's own key stays inert (Q6)
    p = tmp_path / "app_imgproc.yaml"
    for good in (4, 5, 6):
        p.write_text(text + "\nlk_pyramid_levels: %d\n" % good)
        assert load(p) == (0, good)
    p.write_text(text + "\nlk_pyramid_levels: 8\n")
    assert load(p, 3840, 2160) == (0, 8)
    for bad in ("3", "9", "0", "-5", "5.5", "six", "6 levels", "nan"):
        p.write_text(text + "\nlk_pyramid_levels: %s\n" % bad)
        assert load(p)[0] == -1, bad
        assert b"4 .. 8" in L.mskfh_load_lk_levels_error()
    p.write_text(text + "\nlk_pyramid_levels: 7\n")
    assert load(p)[0] == -1 and b"at most 6" in L.mskfh_load_lk_levels_error()      # 752 x 480 allows up to 6
    assert load(p, 239, 120)[0] == -1 and b"at most 4" in L.mskfh_load_lk_levels_error()
    assert load(p, 1920, 1080) == (0, 7)
