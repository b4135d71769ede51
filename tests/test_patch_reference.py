"""The patch-check contract ("Patch check") on the CPU: known answers of the numpy restatement
(tests/patch_reference.py), csrc/hip/fe_patch.h (the header the kernel and the C ABI run) compiled with g++ == the restatement,
sum for sum and bit for bit, at the borders of the images and of the coordinate rule, the deliberate mistakes of
patch_reference.MUTATIONS, each of which changes some expected output of these cases, the scenes the GPU tests use (chosen
here, with the oracle's LK, so that what they expect holds before a GPU is asked) and the YAML keys of the host mirror."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import patch_reference as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(17, 17), (40, 33), (188, 120)]        # w, h
HALVES = [2, 4, 7]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("fe_patch") / "libfe_patch_test.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-shared", "-fPIC", "-I", ROOT, "-o", so,
                           os.path.join(ROOT, "tests", "cpp", "fe_patch_test.cpp")])
    L = C.CDLL(so)
    L.fp_thr2_of.argtypes = [C.c_float]
    L.fp_thr2_of.restype = C.c_double
    L.fp_coord_of.argtypes = [C.c_float, C.c_int, C.c_void_p]
    L.fp_coord_of.restype = None
    L.fp_compare.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int, C.c_double, C.c_void_p]
    L.fp_gate_points.argtypes = [C.c_void_p] * 3 + [C.c_int] * 4 + [C.c_float] * 2 + [C.c_int] * 2 + [C.c_void_p] * 6
    L.fp_gate_points.restype = None

    class H:
        lib = L

        @staticmethod
        def compare(img_a, xa, ya, img_b, xb, yb, half, t2):
            """(sums (n, 5) int64, decisions bool) of the header, point by point."""
            img_a, img_b = np.ascontiguousarray(img_a, np.uint8), np.ascontiguousarray(img_b, np.uint8)
            n = len(xa)
            s, ok = np.zeros((n, 5), np.uint32), np.zeros(n, bool)
            for i in range(n):
                ok[i] = L.fp_compare(img_a.ctypes.data, img_a.shape[1], img_a.shape[0], float(xa[i]), float(ya[i]), img_b.ctypes.data, img_b.shape[1], img_b.shape[0],
                                     float(xb[i]), float(yb[i]), half, float(t2), s[i].ctypes.data) != 0
            return s.astype(np.int64), ok

        @staticmethod
        def gate(prev0, curr0, curr1, mode, half, tt, ts, do_temporal, in_pts, out0, out1, und0, und1, status):
            imgs = [np.ascontiguousarray(x, np.uint8) for x in (prev0, curr0, curr1)]
            h, w = imgs[0].shape
            pin = np.array(in_pts, np.float32).reshape(-1, 2)
            a = [np.array(x, np.float32).reshape(-1, 2) for x in (out0, out1, und0, und1)]
            st = np.array(status, np.uint8)
            L.fp_gate_points(*[x.ctypes.data for x in imgs], w, h, mode, half, float(tt), float(ts), int(do_temporal), len(st), pin.ctypes.data,
                             *[x.ctypes.data for x in a], st.ctypes.data)
            return (*a, st)
    return H


# ------------------------------------------------------------------------------------------ images and points
def texture(w, h, seed):
    """A random texture with structure at several scales (so that neighbouring patches correlate a little, not fully)."""
    rng = np.random.default_rng([w, h, seed])
    img = rng.integers(0, 256, (h, w)).astype(np.float64)
    coarse = np.kron(rng.integers(0, 256, ((h + 3) // 4, (w + 3) // 4)), np.ones((4, 4)))[:h, :w]
    return np.clip(0.5 * img + 0.5 * coarse, 0, 255).astype(np.uint8)


def image_pair(w, h, seed):
    """(A, B): B is A moved by (2, 1) pixels with gain, offset and noise that grows from left to right: points of A at (x, y)
    against points of B at (x + 2, y + 1) correlate well on the left and badly on the right."""
    a = texture(w, h, seed)
    rng = np.random.default_rng([w, h, seed, 1])
    moved = np.roll(np.roll(a, 1, 0), 2, 1).astype(np.float64)
    noise = rng.standard_normal((h, w)) * np.linspace(0, 90, w)[None, :]
    b = np.clip(0.8 * moved + 20 + noise, 0, 255).astype(np.uint8)
    return a, b


def edge_points(w, h):
    """(n, 2) float32: the four corners, a point on every edge, x = W - 1 exactly, fractions 0, 31 / 32 and 0.99, negative and NaN
    coordinates, and points inside."""
    f31, nan = 31.0 / 32.0, float("nan")
    pts = [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1), (w // 2, 0), (w // 2 + 0.5, h - 1), (0, h // 2 + 0.25), (w - 1, h // 2),
           (w - 1, 3.5), (w - 1 - f31, 5 + f31), (w - 2 + f31, h - 2 + f31), (5.0, 6.0), (5 + f31, 6.0), (5.0, 6 + f31), (5.99, 6.99), (7.515625, 8.484375),
           (-3.5, 4.0), (4.0, -0.25), (-1e9, -1e9), (nan, 5.0), (6.0, nan), (nan, nan), (w + 10.0, h + 10.0), (1e9, 2.0), (0.999, 0.001),
           (w / 2 + 0.3, h / 2 + 0.7), (w / 3, h / 3), (2 * w / 3 + 0.111, h / 4 + 0.889)]
    return np.array(pts, np.float32)


def _flat(v, w=24, h=24):
    return np.full((h, w), v, np.uint8)


# ------------------------------------------------------------------------------------------ known answers
def test_coordinate_rule(harness):
    out = (C.c_int * 2)()
    for x, size, want in [(0.0, 17, (0, 0)), (16.0, 17, (16, 0)), (16.9, 17, (16, 0)), (-2.0, 17, (0, 0)), (float("nan"), 17, (0, 0)), (5.96875, 17, (5, 31)),
                          (5.99, 17, (5, 31)), (5.5, 17, (5, 16)), (5.03, 17, (5, 0)), (1e9, 188, (187, 0)), (186.999, 188, (186, 31))]:
        ix, ax = PR.coord(np.float32(x), size)
        harness.lib.fp_coord_of(float(np.float32(x)), size, out)
        assert (int(ix[0]), int(ax[0])) == want == (out[0], out[1]), x
    assert harness.lib.fp_half_min() == PR.MIN_HALF and harness.lib.fp_half_max() == PR.MAX_HALF
    for t in (0.0, 0.8, 1.0, 0.33333334):
        assert harness.lib.fp_thr2_of(t) == PR.thr2(t)
    assert PR.thr2(0.8) == float(np.float32(0.8)) ** 2 != 0.8 ** 2


def test_a_patch_against_itself_passes_at_one():
    img = texture(40, 33, 1)
    pts = edge_points(40, 33)
    for half in HALVES:
        s = PR.sums(img, pts[:, 0], pts[:, 1], img, pts[:, 0], pts[:, 1], half)
        assert PR.decide(s, half, PR.thr2(1.0)).all()
        num, va, vb = PR.terms(s, half)
        assert np.array_equal(num, va) and np.array_equal(va, vb) and (va > 0).all()


def test_gain_and_offset_pass_at_one():
    """B = 2 A + 10 without clipping at integer coordinates: v = 4 I exactly, so num^2 == va vb, and >= lets it pass at 1.0."""
    a = (texture(40, 33, 2) // 3).astype(np.uint8)                    # 0 .. 85
    b = (2 * a.astype(np.int64) + 10).astype(np.uint8)
    pts = np.array([(10, 10), (20, 16), (0, 0), (39, 32), (7, 30)], np.float32)
    for half in HALVES:
        assert np.array_equal(PR.samples(a, pts[:, 0], pts[:, 1], half)[0], 4 * a[10 - half:10 + half + 1, 10 - half:10 + half + 1].astype(np.int64))
        s = PR.sums(a, pts[:, 0], pts[:, 1], b, pts[:, 0], pts[:, 1], half)
        num, va, vb = PR.terms(s, half)
        assert np.array_equal(num * num, va * vb) and (num > 0).all()          # (exact in Python integers)
        assert all(int(n) ** 2 == int(x) * int(y) for n, x, y in zip(num, va, vb))
        assert PR.decide(s, half, PR.thr2(1.0)).all()
        assert not PR.decide(s, half, PR.thr2(1.0), mutate="gt").any()


def test_inverted_patch_fails_at_zero():
    a = texture(40, 33, 3)
    b = (255 - a).astype(np.uint8)
    pts = edge_points(40, 33)
    for half in HALVES:
        s = PR.sums(a, pts[:, 0], pts[:, 1], b, pts[:, 0], pts[:, 1], half)
        assert (PR.terms(s, half)[0] < 0).all()
        assert not PR.decide(s, half, PR.thr2(0.0)).any()


def test_flat_patches():
    tex = texture(24, 24, 4)
    pts = np.array([(12, 12), (11.5, 12.25)], np.float32)
    for half in HALVES:
        both = PR.sums(_flat(90), pts[:, 0], pts[:, 1], _flat(200), pts[:, 0], pts[:, 1], half)
        assert PR.decide(both, half, PR.thr2(1.0)).all()                        # nothing to judge
        for a, b in ((_flat(90), tex), (tex, _flat(90))):
            one = PR.sums(a, pts[:, 0], pts[:, 1], b, pts[:, 0], pts[:, 1], half)
            assert (PR.terms(one, half)[0] == 0).all()
            assert not PR.decide(one, half, PR.thr2(0.0)).any()


SHIFT_SEED = 5


def test_shifted_random_texture_fails():
    rng = np.random.default_rng(SHIFT_SEED)
    img = rng.integers(0, 256, (33, 40)).astype(np.uint8)
    x, y = np.arange(8, 32, 3, dtype=np.float32), np.full(8, 16, np.float32)
    for half in HALVES:
        for dx, dy in ((1, 0), (0, 1)):
            s = PR.sums(img, x, y, img, x + dx, y + dy, half)
            assert not PR.decide(s, half, PR.thr2(0.8)).any()
            assert (np.abs(PR.zncc(s, half)) < 0.6).all()


def test_sums_fit_32_bits(harness):
    """The largest sums there are: all-255 patches at half 7; and the 255 / 0 chequer against its inverse."""
    yy, xx = np.mgrid[0:24, 0:24]
    chq = np.where((xx + yy) % 2 == 0, 255, 0).astype(np.uint8)
    inv = (255 - chq).astype(np.uint8)
    pts = np.array([(12, 12), (12.5, 12.5)], np.float32)
    for a, b in ((_flat(255), _flat(255)), (chq, inv), (chq, chq), (_flat(255), chq)):
        want = PR.sums(a, pts[:, 0], pts[:, 1], b, pts[:, 0], pts[:, 1], 7)
        assert (want < 2 ** 32).all() and (want >= 0).all()
        got, ok = harness.compare(a, pts[:, 0], pts[:, 1], b, pts[:, 0], pts[:, 1], 7, PR.thr2(0.8))
        assert np.array_equal(got, want) and np.array_equal(ok, PR.decide(want, 7, PR.thr2(0.8)))
    top = PR.sums(_flat(255), pts[:1, 0], pts[:1, 1], _flat(255), pts[:1, 0], pts[:1, 1], 7)[0]
    assert list(top) == [225 * 1020, 225 * 1020] + [225 * 1020 * 1020] * 3 and 225 * 1020 * 1020 < 2 ** 32
    s = PR.sums(chq, pts[:1, 0], pts[:1, 1], inv, pts[:1, 0], pts[:1, 1], 7)
    assert s[0, 4] == 0 and not PR.decide(s, 7, PR.thr2(0.0))[0]


# ------------------------------------------------------------------------------------------ the header == the restatement
THRESHOLDS = [0.0, 0.5, 0.8, 0.95, 1.0]


def comparison_cases(w, h):
    """(name, A, pts_a, B, pts_b) over which the header and the restatement are compared."""
    a, b = image_pair(w, h, 7)
    pts = edge_points(w, h)
    moved = pts + np.array([2, 1], np.float32)
    bright = np.clip(200 + (texture(w, h, 9).astype(np.int64) - 128) // 16, 0, 255).astype(np.uint8)       # low contrast on a high mean
    return [("self", a, pts, a, pts), ("pair", a, pts, b, moved), ("pair_unmoved", a, pts, b, pts), ("inverted", a, pts, (255 - a).astype(np.uint8), pts),
            ("bright", bright, pts, bright, pts), ("flat_vs_texture", np.full((h, w), 77, np.uint8), pts, a, pts)]


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_header_equals_restatement(harness, size):
    w, h = size
    decided = []
    for name, a, pa, b, pb in comparison_cases(w, h):
        for half in HALVES:
            want = PR.sums(a, pa[:, 0], pa[:, 1], b, pb[:, 0], pb[:, 1], half)
            for t in THRESHOLDS:
                got, ok = harness.compare(a, pa[:, 0], pa[:, 1], b, pb[:, 0], pb[:, 1], half, PR.thr2(t))
                assert np.array_equal(got, want), (name, half)
                assert np.array_equal(ok, PR.decide(want, half, PR.thr2(t))), (name, half, t)
                decided.append(ok)
    decided = np.concatenate(decided)
    assert decided.sum() > 100 and (~decided).sum() > 100


def gate_images(w, h, seed):
    """(prev0, curr0, curr1): curr0 is prev0 moved by (2, 1) with noise growing to the right (image_pair), curr1 is curr0 moved by
    another (2, 1) on half of its pixels and a noisy other texture on the rest."""
    prev0, curr0 = image_pair(w, h, seed)
    other = image_pair(w, h, seed + 100)[1]
    curr1 = np.where(np.random.default_rng([seed, 2]).random((h, w)) < 0.5, np.roll(np.roll(curr0, 1, 0), 2, 1), other).astype(np.uint8)
    return prev0, curr0, curr1


def gate_points(w, h, n, seed, do_temporal):
    """Synthetic track outputs for gate_images: (in_pts, out0, out1, und0, und1, status) of n points; the points are those of
    edge_points and random ones (half of them on quarter pixels), out0 = in_pts + (2, 1) and out1 = out0 + (2, 1) with a jitter."""
    rng = np.random.default_rng([w, h, n, seed])
    base = edge_points(w, h)
    rnd = np.stack([rng.uniform(-2, w + 1, max(n, 1)), rng.uniform(-2, h + 1, max(n, 1))], 1).astype(np.float32)
    rnd[::2] = np.floor(rnd[::2] * 4) / 4
    pin = np.concatenate([base, rnd])[np.arange(n) % (len(base) + len(rnd))] if n else np.zeros((0, 2), np.float32)
    out0 = (pin + np.array([2, 1], np.float32) + rng.uniform(-0.3, 0.3, (n, 2)).astype(np.float32)).astype(np.float32)
    out1 = (out0 + np.array([2, 1], np.float32) + rng.uniform(-0.3, 0.3, (n, 2)).astype(np.float32)).astype(np.float32)
    und0, und1 = rng.standard_normal((n, 2)).astype(np.float32), rng.standard_normal((n, 2)).astype(np.float32)
    status = rng.choice(np.array([0, 1, 3, 3, 3], np.uint8), n) if do_temporal else rng.choice(np.array([0, 3, 3, 3], np.uint8), n)
    return pin, out0, out1, und0, und1, status.astype(np.uint8)


def gate_case(w, h, n, seed, do_temporal):
    return (*gate_images(w, h, seed), *gate_points(w, h, n, seed, do_temporal))


GATE_T = (0.35, 0.3)          # thresholds near the medians of gate_case: about half of the points fail each comparison


@pytest.mark.parametrize("size", SIZES[:2], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("mode", [1, 2, 3, 0])
def test_gate_header_equals_restatement(harness, size, mode):
    w, h = size
    for do_temporal in (1, 0):
        for half in HALVES:
            prev0, curr0, curr1, *arrs = gate_case(w, h, 120, 3 * half + do_temporal, do_temporal)
            want = PR.gate(prev0, curr0, curr1, mode, half, GATE_T[0], GATE_T[1], do_temporal, *arrs)
            got = harness.gate(prev0, curr0, curr1, mode, half, GATE_T[0], GATE_T[1], do_temporal, *arrs)
            for a, b in zip(want, got):
                assert a.tobytes() == b.tobytes()
            pin, out0, out1, und0, und1, status = arrs
            assert want[0].tobytes() == out0.tobytes()                             # out0 is always kept (NaNs included)
            lost = (status != 0) & (want[4] == 0)
            unmatched = (status == 3) & (want[4] == 1)
            assert lost.any() == bool(mode & 1 and do_temporal) and unmatched.any() == bool(mode & 2)
            assert np.all(want[1][lost] == 0) and np.all(want[2][lost] == 0) and np.all(want[3][lost] == 0)
            keep = ~lost
            assert want[1][keep].tobytes() == out1[keep].tobytes() and np.array_equal(want[2][keep], und0[keep]) and np.array_equal(want[3][keep], und1[keep])
            assert (want[4][keep] != 0).sum() > 10                                 # ... and not everything goes


def equality_half():
    """(A, B, x, y): 5 x 5 patches at (12, 12) whose correlation is 0.5 exactly: A = 100 + 10 u, B = 100 + 10 (u + r) with u a
    zero-sum column pattern of energy 20 and r a zero-sum row pattern of energy 60, orthogonal to it."""
    u = np.array([1, -1, 0, 1, -1])[None, :] * np.ones((5, 1), np.int64)
    r = np.array([3, -1, -1, -1, 0])[:, None] * np.ones((1, 5), np.int64)
    a, b = np.full((24, 24), 100, np.int64), np.full((24, 24), 100, np.int64)
    a[10:15, 10:15] += 10 * u
    b[10:15, 10:15] += 10 * (u + r)
    return a.astype(np.uint8), b.astype(np.uint8), np.array([12], np.float32), np.array([12], np.float32)


def test_equality_passes(harness):
    """num^2 == thr2 va vb exactly passes (>=): at threshold 1.0 with gain and offset, at 0.5 with the constructed patches."""
    a = (texture(40, 33, 2) // 3).astype(np.uint8)
    b = (2 * a.astype(np.int64) + 10).astype(np.uint8)
    x, y = np.array([10, 20], np.float32), np.array([10, 16], np.float32)
    for half in HALVES:
        got, ok = harness.compare(a, x, y, b, x, y, half, PR.thr2(1.0))
        assert ok.all() and PR.decide(got, half, PR.thr2(1.0)).all()
    a, b, x, y = equality_half()
    s = PR.sums(a, x, y, b, x, y, 2)
    num, va, vb = (int(v[0]) for v in PR.terms(s, 2))
    assert num > 0 and 4 * num * num == va * vb and PR.thr2(0.5) == 0.25
    got, ok = harness.compare(a, x, y, b, x, y, 2, PR.thr2(0.5))
    assert np.array_equal(got, s) and ok[0] and PR.decide(s, 2, PR.thr2(0.5))[0]
    assert not PR.decide(s, 2, PR.thr2(0.5), mutate="gt")[0]
    above = float(np.nextafter(np.float32(0.5), np.float32(1)))
    assert not PR.decide(s, 2, PR.thr2(above))[0] and not harness.compare(a, x, y, b, x, y, 2, PR.thr2(above))[1][0]


# ------------------------------------------------------------------------------------------ the mistakes would be seen
def _expected_outputs(mutate=None):
    """Everything the comparisons above expect, under one mistake."""
    out = []
    for name, a, pa, b, pb in comparison_cases(40, 33):
        for half in (2, 4):
            s = PR.sums(a, pa[:, 0], pa[:, 1], b, pb[:, 0], pb[:, 1], half, mutate)
            out.append(s.tobytes())
            out += [PR.decide(s, half, PR.thr2(t), mutate).tobytes() for t in THRESHOLDS]
    a = (texture(40, 33, 2) // 3).astype(np.uint8)
    b = (2 * a.astype(np.int64) + 10).astype(np.uint8)
    x, y = np.array([10, 20], np.float32), np.array([10, 16], np.float32)
    s = PR.sums(a, x, y, b, x, y, 4, mutate)
    out.append(PR.decide(s, 4, PR.thr2(1.0), mutate).tobytes())
    return out


@pytest.mark.parametrize("mutate", PR.MUTATIONS)
def test_every_mistake_changes_an_expected_output(mutate):
    want, got = _expected_outputs(), _expected_outputs(mutate)
    assert len(want) == len(got) and any(a != b for a, b in zip(want, got)), mutate


def test_mistakes_in_the_decision_change_decisions():
    """The mistakes that leave the sums alone are seen in the decisions: > for >= at equality, a dropped num > 0 on the inverted
    patch, N = (2 half)^2 on the bright low-contrast patch (N SAA - SA^2 turns negative)."""
    want, got = _expected_outputs(), {m: _expected_outputs(m) for m in ("gt", "no_num_positive", "n_even")}
    for m, g in got.items():
        changed = [k for k, (a, b) in enumerate(zip(want, g)) if a != b]
        assert changed and all(k % 6 != 0 or k == len(want) - 1 for k in changed), m          # (every sixth entry is a block of sums)


# ------------------------------------------------------------------------------------------ the scenes of the GPU tests, chosen here
REAL = dict(w=188, h=120, seed=0x5EED00C0, frame=30, half=4)


def real_track_points(cm):
    """The points test_gpu_patch tracks: cell maxima (cell_maxima records) above the detector threshold, the first 200."""
    return np.stack([cm["x"], cm["y"]], 1)[cm["score"] > 2560][:200].astype(np.float32)


def median_threshold(z):
    """A float32 threshold in [0, 1] that at least ten of the values z miss and at least ten reach, or None."""
    z = np.sort(np.asarray(z, np.float64))
    if len(z) < 20:
        return None
    t = np.float32(np.clip(z[len(z) // 2], 0, 1))
    return float(t) if (z < t).sum() >= 10 and (z >= t).sum() >= 10 and 0 < t < 1 else None


def test_thresholds_exist_for_the_real_track(oracle):
    """With the oracle's LK on the frames test_gpu_patch tracks: the ZNCC of the surviving points spreads enough that a threshold
    fails ten and passes ten, in the temporal and in both stereo comparisons."""
    w, h, half = REAL["w"], REAL["h"], REAL["half"]
    syn = oracle.Synth(seed=REAL["seed"], width=w, height=h)
    (a0, b0), (a1, b1) = syn.render(REAL["frame"]), syn.render(REAL["frame"] + 1)
    pts = real_track_points(oracle.cell_maxima(a0))
    assert len(pts) > 40
    out0, st = oracle.lk_track(a0, a1, pts, pts)
    k = np.flatnonzero(st)
    assert median_threshold(PR.zncc(PR.sums(a0, pts[k, 0], pts[k, 1], a1, out0[k, 0], out0[k, 1], half), half)) is not None
    from msckf_stereo_c_amd.ctypes_types import default_fe_cfg
    for img0, img1, p in ((a1, b1, out0[k]), (a0, b0, pts)):
        o1, m = oracle.stereo_match(syn.calib, default_fe_cfg(), img0, img1, p)
        kk = np.flatnonzero(m)
        assert median_threshold(PR.zncc(PR.sums(img0, p[kk, 0], p[kk, 1], img1, o1[kk, 0], o1[kk, 1], half), half)) is not None


OCCLUDER = dict(w=188, h=120, seed=0x5EED00F0, n_frames=30, box=(30, 90, 60, 130))          # box: y0, y1, x0, x1 of cam1


def occlude(cam1):
    """cam1 with a block of foreign texture (uniform noise) pasted over OCCLUDER["box"]."""
    y0, y1, x0, x1 = OCCLUDER["box"]
    out = cam1.copy()
    out[y0:y1, x0:x1] = np.random.default_rng(7).integers(0, 256, (y1 - y0, x1 - x0)).astype(np.uint8)
    return out


def inside_occluder(c1):
    """bool: the features (records with x, y) whose cam1 pixel lies in the pasted block."""
    y0, y1, x0, x1 = OCCLUDER["box"]
    px, py = (c1["x"] + np.float32(0.5)).astype(np.int64), (c1["y"] + np.float32(0.5)).astype(np.int64)
    return (px >= x0) & (px < x1) & (py >= y0) & (py < y1)


def test_the_unchecked_pipeline_publishes_features_on_the_occluder(oracle):
    """The oracle (which has no patch check) publishes at least five features per frame whose cam1 point lies on the pasted block,
    and none of them reaches ZNCC 0.8 against its cam0 patch: the check at its defaults has something to remove."""
    from msckf_stereo_c_amd.ctypes_types import default_ekf_cfg, default_fe_cfg
    w, h, n = OCCLUDER["w"], OCCLUDER["h"], OCCLUDER["n_frames"]
    syn = oracle.Synth(seed=OCCLUDER["seed"], width=w, height=h)
    system = oracle.OracleSystem(syn.calib, default_fe_cfg(), default_ekf_cfg(max_cam_state_size=10))
    j = 0
    for k in range(n):
        t = syn.frame_time(k)
        while True:
            s = syn.imu(j)
            j += 1
            system.imu(s)
            if not (s.time_stamp <= t):
                break
        a, b = syn.render(k)
        b = occlude(b)
        system.stereo(a, b, t)
        system.backend()
        ids, life, c0, c1, info = system.dump()
        ins = inside_occluder(c1)
        assert ins.sum() >= 5, k
        z = PR.zncc(PR.sums(a, c0["x"][ins], c0["y"][ins], b, c1["x"][ins], c1["y"][ins], 4), 4)
        assert (z < 0.7).all(), k


# ------------------------------------------------------------------------------------------ the YAML keys
def test_patch_check_yaml_keys(tmp_path):
    from msckf_stereo_c_amd import build
    from msckf_stereo_c_amd.ctypes_types import FePatchCheck
    build.build_all()
    L = C.CDLL(os.path.join(ROOT, "msckf_stereo_c_amd", "_build", "libmskf_host.so"))
    L.mskfh_load_patch_check.argtypes = [C.c_char_p, C.POINTER(FePatchCheck)]

    def load(path):
        c = FePatchCheck(-1, -1, -1.0, -1.0)
        rc = L.mskfh_load_patch_check(str(path).encode(), C.byref(c))
        return rc, c.mode, c.half, c.min_zncc_temporal, c.min_zncc_stereo
    stock = os.path.join(ROOT, "config", "app_imgproc.yaml")
    f08 = float(np.float32(0.8))
    assert load(stock) == (0, 0, 4, f08, f08)                          # absent means off, with the documented defaults
    text = open(stock).read()
    p = tmp_path / "app_imgproc.yaml"
    for name, mode in (("off", 0), ("temporal", 1), ("stereo", 2), ("both", 3)):
        p.write_text(text + "\npatch_check: %s\npatch_check_half: 6\npatch_check_min_zncc_temporal: 0.75\npatch_check_min_zncc_stereo: 0.5\n" % name)
        assert load(p) == (0, mode, 6, 0.75, 0.5)
    p.write_text(text + "\npatch_check: both\n")
    assert load(p) == (0, 3, 4, f08, f08)
    p.write_text(text + "\npatch_check: sometimes\n")
    assert load(p)[0] == -1
