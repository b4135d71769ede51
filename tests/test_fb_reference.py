"""The forward-backward contract ("Forward-backward check") on the CPU: csrc/hip/fe_fb.h (the header the kernel
and the C ABI run) compiled with g++ == the numpy restatement (tests/fb_reference.py) at the edges of the decision, the
deliberate mistakes of fb_reference.MUTATIONS, each of which changes some expected output of these cases, the inputs of the GPU
tests (chosen here, on the oracle's LK alone, so that what they expect holds before a GPU is asked), the occluder scene at the
defaults, and the YAML keys of the host mirror."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import fb_reference as FB
from test_patch_reference import OCCLUDER

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class FeFbDev(C.Structure):
    """FeFbDev of csrc/hip/fe_fb.h: element i goes with descriptor i of a launch."""
    _fields_ = [("thr2_t", C.c_float), ("thr2_s", C.c_float), ("mode", C.c_int)]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("fe_fb") / "libfe_fb_test.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-shared", "-fPIC", "-I", ROOT, "-o", so,
                           os.path.join(ROOT, "tests", "cpp", "fe_fb_test.cpp")])
    L = C.CDLL(so)
    L.fb_max_error.restype = C.c_float
    L.fb_thr2_of.argtypes = [C.c_float]
    L.fb_thr2_of.restype = C.c_float
    L.fb_pass_points.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p]
    L.fb_pass_points.restype = None

    class H:
        lib = L

        @staticmethod
        def fb_pass(bx, by, ox, oy, st, t2):
            back = np.ascontiguousarray(np.stack([bx, by], 1), np.float32)
            origin = np.ascontiguousarray(np.stack([ox, oy], 1), np.float32)
            st = np.ascontiguousarray(st, np.uint8)
            out = np.zeros(len(st), np.uint8)
            L.fb_pass_points(len(st), back.ctypes.data, origin.ctypes.data, st.ctypes.data, C.c_float(float(t2)), out.ctypes.data)
            return out != 0
    return H


def test_fe_fb_dev_layout_and_constants(harness):
    from msckf_stereo_c_amd.ctypes_types import FB_CHECK_MODES, FB_MAX_ERROR, FeFbCheck
    out = (C.c_int * 8)()
    n = harness.lib.fb_dev_layout(out, 8)
    assert list(out[:n]) == [C.sizeof(FeFbDev)] + [getattr(FeFbDev, k).offset for k in ("thr2_t", "thr2_s", "mode")] == [12, 0, 4, 8]
    assert harness.lib.fb_max_error() == FB.MAX_ERROR == FB_MAX_ERROR
    assert harness.lib.fb_mode_bits() == FB.TEMPORAL | (FB.STEREO << 8)
    assert FB_CHECK_MODES == {"off": 0, "temporal": FB.TEMPORAL, "stereo": FB.STEREO, "both": FB.TEMPORAL | FB.STEREO}
    assert C.sizeof(FeFbCheck) == 12 and [f[0] for f in FeFbCheck._fields_] == ["mode", "max_error_temporal", "max_error_stereo"]
    for t in (0.0, 1.0, 0.8, 0.1, 1.7, 64.0, 0.33333334):
        assert harness.lib.fb_thr2_of(t) == FB.thr2(t) and isinstance(FB.thr2(t), np.float32)
    assert FB.thr2(0.1) == np.float32(0.1) * np.float32(0.1) != np.float32(0.1 * 0.1)


# ------------------------------------------------------------------------------------------ the decision at its edges
def _f32(x):
    return np.float32(x)


def _up(x):
    return np.nextafter(np.float32(x), np.float32(np.inf))


def _down(x):
    return np.nextafter(np.float32(x), np.float32(-np.inf))


def double_rounding_case():
    """(dx, dy, t): float32 values whose squared distance rounds DOWN onto t * t in float32 (passes) and lies above it in double
    (the "double" mistake fails it).  Found by a fixed search, so the case is what the arithmetic says and not a stored number."""
    t = np.float32(1.7)
    t2 = FB.thr2(t)
    for dy in np.arange(0.25, 1.25, 1.0 / 64, dtype=np.float32):
        dx = np.float32(np.sqrt(np.float64(t2) - np.float64(dy) ** 2) - 2e-6)
        for _ in range(40):
            d32 = np.float32(np.float32(dx * dx) + np.float32(dy * dy))
            if d32 == t2 and np.float64(dx) ** 2 + np.float64(dy) ** 2 > np.float64(t2):
                return dx, dy, t
            dx = _up(dx)
    raise AssertionError("no double-rounding case near 1.7")


def decision_cases():
    """(bx, by, ox, oy, st, t2, want) arrays: the edges of fb_pass."""
    nan, inf = np.float32("nan"), np.float32("inf")
    rows = []

    def add(bx, by, ox, oy, st, t, want):
        rows.append((_f32(bx), _f32(by), _f32(ox), _f32(oy), st, FB.thr2(t), want))
    # equality exactly at the threshold passes: a 3-4-5 triangle, and 0.75 / 1.0 / 1.25 (all exact in float32)
    add(13, 24, 10, 20, 1, 5.0, True)
    add(10.75, 21, 10, 20, 1, 1.25, True)
    add(7, 20, 10, 24, 1, 5.0, True)
    # one ulp above it fails: the coordinate a step further out, or the threshold a step lower
    add(_up(13), 24, 10, 20, 1, 5.0, False)
    add(13, _up(24), 10, 20, 1, 5.0, False)
    add(13, 24, 10, 20, 1, _down(5.0), False)
    add(_down(13), 24, 10, 20, 1, 5.0, True)
    # NaN and infinite coordinates fail, whatever the threshold
    for t in (0.0, 1.0, 64.0):
        add(nan, 20, 10, 20, 1, t, False)
        add(10, nan, 10, 20, 1, t, False)
        add(10, 20, nan, 20, 1, t, False)
        add(10, 20, 10, nan, 1, t, False)
        add(inf, 20, 10, 20, 1, t, False)
        add(10, -inf, 10, 20, 1, t, False)
        add(inf, 20, inf, 20, 1, t, False)              # inf - inf = NaN
    # st == 0 fails, even an exact return; any other status value counts as success
    add(10, 20, 10, 20, 0, 1.0, False)
    add(10, 20, 10, 20, 0, 64.0, False)
    add(10, 20, 10, 20, 1, 1.0, True)
    add(10, 20, 10, 20, 255, 1.0, True)
    # threshold 0 passes only an exact return
    add(10, 20, 10, 20, 1, 0.0, True)
    add(_up(10), 20, 10, 20, 1, 0.0, False)
    add(10, _down(20), 10, 20, 1, 0.0, False)
    add(-0.0, 0.0, 0.0, -0.0, 1, 0.0, True)
    # a distance so small that its square underflows to 0 passes at threshold 0 (dx * dx rounds to 0 in float32)
    add(1e-30, 0, 0, 0, 1, 0.0, True)
    # the largest legal threshold: 64 px, 4096 squared
    add(74, 20, 10, 20, 1, 64.0, True)
    add(_up(74), 20, 10, 20, 1, 64.0, False)
    add(10, 84.5, 10, 20, 1, 64.0, False)
    add(48, 71, 10, 20, 1, 64.0, True)
    add(1e20, 20, 10, 20, 1, 64.0, False)              # the square overflows to inf
    # float32 rounding decides: see double_rounding_case
    dx, dy, t = double_rounding_case()
    rows.append((dx, dy, _f32(0), _f32(0), 1, FB.thr2(t), True))
    cols = list(zip(*rows))
    return [np.array(c, np.float32) for c in cols[:4]] + [np.array(cols[4], np.uint8), np.array(cols[5], np.float32), np.array(cols[6], bool)]


def _decide(cases, fn):
    bx, by, ox, oy, st, t2, _ = cases
    return np.array([bool(fn(bx[i:i + 1], by[i:i + 1], ox[i:i + 1], oy[i:i + 1], st[i:i + 1], t2[i])[0]) for i in range(len(st))])


def test_fb_pass_header_equals_restatement_at_the_edges(harness):
    cases = decision_cases()
    want = cases[6]
    assert np.array_equal(_decide(cases, FB.fb_pass), want)
    assert np.array_equal(_decide(cases, harness.fb_pass), want)
    assert want.sum() >= 8 and (~want).sum() >= 8
    # ... and on a cloud of round trips around each threshold
    rng = np.random.default_rng(5)
    for t in (0.0, 0.5, 1.0, 2.0, 64.0):
        o = rng.uniform(-5, 200, (4000, 2)).astype(np.float32)
        b = (o + rng.normal(0, max(t, 0.01), (4000, 2)).astype(np.float32)).astype(np.float32)
        b[::50] = o[::50]
        st = rng.choice(np.array([0, 1, 1, 1], np.uint8), 4000)
        a = FB.fb_pass(b[:, 0], b[:, 1], o[:, 0], o[:, 1], st, FB.thr2(t))
        assert np.array_equal(a, harness.fb_pass(b[:, 0], b[:, 1], o[:, 0], o[:, 1], st, FB.thr2(t)))
        assert a.sum() > 20 and (~a & (st != 0)).sum() > 20


# ------------------------------------------------------------------------------------------ the inputs of the GPU tests, chosen here
DIRECT_SIZES = [(65, 67), (129, 71)]          # w, h: level 3 is 9 x 9 and 17 x 9
DIRECT_T = (1.0, 0.75)                        # thresholds the jittered round trips straddle
IMG_SEED = 21


def smooth_texture(w, h, seed):
    """A texture with structure at several scales that LK can follow: random grids at 2, 4, 8 and 16 pixels, upsampled and box-
    smoothed, on a little pixel noise."""
    rng = np.random.default_rng([w, h, seed])
    acc = rng.uniform(0, 1, (h, w)) * 0.15
    for cell, gain in ((2, 0.5), (4, 1.0), (8, 1.0), (16, 0.7)):
        g = np.kron(rng.uniform(0, 1, ((h + cell - 1) // cell + 1, (w + cell - 1) // cell + 1)), np.ones((cell, cell)))
        k = cell // 2
        g = np.roll(np.roll(g, rng.integers(0, cell), 0), rng.integers(0, cell), 1)
        for axis in (0, 1):
            g = sum(np.roll(g, s, axis) for s in range(-k, k + 1)) / (2 * k + 1)
        acc += gain * g[:h, :w]
    acc -= acc.min()
    return np.clip(acc / acc.max() * 255, 0, 255).astype(np.uint8)


def gate_images(w, h, seed):
    """(prev0, curr0, curr1): curr0 is prev0 moved by (2, 1), curr1 is curr0 moved by another (2, 1) on half of its pixels (in
    blocks of 16) and foreign texture on the rest."""
    prev0 = smooth_texture(w, h, seed)
    curr0 = np.roll(np.roll(prev0, 1, 0), 2, 1)
    other = smooth_texture(w, h, seed + 100)
    blocks = np.kron(np.random.default_rng([seed, 2]).random(((h + 15) // 16, (w + 15) // 16)) < 0.5, np.ones((16, 16), bool))[:h, :w]
    curr1 = np.where(blocks, np.roll(np.roll(curr0, 1, 0), 2, 1), other).astype(np.uint8)
    return prev0, curr0, curr1


def gate_points(w, h, n, seed, do_temporal, statuses=None):
    """Synthetic track outputs for gate_images: (in_pts, out0, out1, und0, und1, status) of n points spread over the image and
    a little beyond every border; out0 = in_pts + (2, 1) + jitter and out1 = out0 + (2, 1) + jitter, the jitter's length spread over
    0 .. 2 px, so that the round-trip errors straddle DIRECT_T.  Statuses 0 / 1 / 3 are mixed point by point unless given."""
    rng = np.random.default_rng([w, h, n, seed])
    m = max(n, 1)
    pin = np.stack([rng.uniform(-2, w + 1, m), rng.uniform(-2, h + 1, m)], 1).astype(np.float32)[:n]
    pin[::2] = np.floor(pin[::2] * 4) / 4

    def jitter():
        r, a = rng.uniform(0, 2, n), rng.uniform(0, 2 * np.pi, n)
        return np.stack([r * np.cos(a), r * np.sin(a)], 1).astype(np.float32)
    out0 = (pin + np.array([2, 1], np.float32) + jitter()).astype(np.float32)
    out1 = (out0 + np.array([2, 1], np.float32) + jitter()).astype(np.float32)
    und0, und1 = rng.standard_normal((n, 2)).astype(np.float32), rng.standard_normal((n, 2)).astype(np.float32)
    if statuses is None:
        status = rng.choice(np.array([0, 1, 3, 3, 3], np.uint8), n)
    else:
        status = np.array(statuses, np.uint8)[np.arange(n) % len(statuses)]
    return pin, out0, out1, und0, und1, status.astype(np.uint8)


# statuses of whole four-point groups: groups 0 and 1 mix 0 / 1 / 3 inside a wave (rows differ in `alive` on each trip), group 2
# has no row that needs the temporal trip, group 3 none that needs the stereo trip, group 4 nothing at all
GROUP_STATUSES = [0, 1, 3, 3, 3, 0, 1, 3, 0, 0, 0, 0, 1, 1, 0, 1, 0, 0, 0, 0, 3, 3, 3, 3]


def direct_specs():
    """(n, size index, mode, do_temporal, device-side count or None, statuses or None) per descriptor of the direct launch."""
    specs = [(n, 0, 3, 1, None, None) for n in (0, 1, 3, 4, 5, 63, 64, 65, 257)] + [(257, 1, 3, 1, 100, None)]
    k = 0
    for mode in (1, 2, 3):
        for do_temporal in (1, 0):
            specs.append((65, k % 2, mode, do_temporal, None, None))
            k += 1
            if len(specs) == 13:
                specs.append((65, 1, 0, 1, None, None))                  # mode 0 between two checking descriptors
    specs.append((24, 0, 3, 1, None, GROUP_STATUSES))
    specs.append((24, 1, 3, 0, None, GROUP_STATUSES))
    return specs


def direct_case(k, spec):
    """(images, arrays, expected arrays) of descriptor k: the restatement over the first `count` points."""
    n, si, mode, do_temporal, count, statuses = spec
    w, h = DIRECT_SIZES[si]
    images = gate_images(w, h, IMG_SEED)
    arrs = list(gate_points(w, h, n, 1000 + k, do_temporal, statuses))
    m = n if count is None else count
    gated = FB.gate(*images, mode, DIRECT_T[0], DIRECT_T[1], do_temporal, *[a[:m] for a in arrs])
    exp = [arrs[0]] + [np.concatenate([g, a[m:]]) for g, a in zip(gated, arrs[1:])]
    return images, arrs, exp


def test_direct_cases_change_and_keep_points(oracle):
    """Over the descriptors of the direct launch the restatement changes at least 50 statuses and at least 50 points survive;
    each half removes points and keeps points; a mode-0 descriptor and the points past a device-side count are untouched; the
    round trips leave the image backwards somewhere (status 0 from LK) and the group cases do what their names say."""
    changed = survived = lost_t = lost_s = back_failed = 0
    for k, spec in enumerate(direct_specs()):
        n, si, mode, do_temporal, count, statuses = spec
        images, arrs, exp = direct_case(k, spec)
        m = n if count is None else count
        assert exp[1].tobytes() == arrs[1].tobytes()                             # out0 is always kept
        assert all(e[m:].tobytes() == a[m:].tobytes() for e, a in zip(exp, arrs))
        if mode == 0:
            assert all(e.tobytes() == a.tobytes() for e, a in zip(exp, arrs))
        before, after = arrs[5], exp[5]
        changed += int((before != after).sum())
        survived += int((after[:m] != 0).sum())
        lost = (before != 0) & (after == 0)
        lost_t += int(lost.sum())
        lost_s += int(((before == 3) & (after == 1)).sum())
        assert np.all(exp[2][lost] == 0) and np.all(exp[3][lost] == 0) and np.all(exp[4][lost] == 0)
        keep = ~lost
        assert all(e[keep].tobytes() == a[keep].tobytes() for e, a in zip(exp[2:5], arrs[2:5]))
        assert not lost.any() or (mode & 1 and do_temporal)
        if mode & 1 and do_temporal and n >= 63:
            k1 = np.flatnonzero(before[:m] & 1)
            back_failed += int((FB.round_trip(images[1], images[0], arrs[1][k1], arrs[0][k1])[1] == 0).sum())
    assert changed >= 50 and survived >= 50, (changed, survived)
    assert lost_t >= 20 and lost_s >= 20, (lost_t, lost_s)
    assert back_failed >= 3, back_failed
    # the jitter straddles the thresholds: of the well-textured interior, some round trips end below and some above
    w, h = DIRECT_SIZES[1]
    images = gate_images(w, h, IMG_SEED)
    pin, out0, *_ = gate_points(w, h, 257, 1, 1)
    err, st = FB.round_trip(images[1], images[0], out0, pin)
    ok = st != 0
    assert (err[ok] < DIRECT_T[0]).sum() >= 40 and (err[ok] > DIRECT_T[0]).sum() >= 40


# ------------------------------------------------------------------------------------------ the mistakes would be seen
def _expected_outputs(mutate=None):
    cases = decision_cases()
    out = [_decide(cases, lambda *a: FB.fb_pass(*a, mutate=mutate)).tobytes()]
    for k, spec in enumerate(direct_specs()):
        if spec[0] != 65:
            continue
        n, si, mode, do_temporal, count, statuses = spec
        w, h = DIRECT_SIZES[si]
        arrs = gate_points(w, h, n, 1000 + k, do_temporal, statuses)
        out += [a.tobytes() for a in FB.gate(*gate_images(w, h, IMG_SEED), mode, DIRECT_T[0], DIRECT_T[1], do_temporal, *arrs, mutate=mutate)]
    return out


@pytest.mark.parametrize("mutate", FB.MUTATIONS)
def test_every_mistake_changes_an_expected_output(oracle, mutate):
    want, got = _expected_outputs(), _expected_outputs(mutate)
    assert len(want) == len(got) and any(a != b for a, b in zip(want, got)), mutate
    if mutate != "wrong_origin":
        assert want[0] != got[0], mutate                    # the mistakes in fb_pass itself are seen in the decision cases already
    else:
        assert want[0] == got[0] and any(a != b for a, b in zip(want[1:], got[1:]))


# ------------------------------------------------------------------------------------------ the occluder scene at the defaults
REAL_FRAMES = (5, 6)
# The scene is OCCLUDER's with the next seed.  With OCCLUDER's own seed the unoccluded stereo pair holds one genuinely wrong match
# (the point (168, 110), ten pixels from the lower border, matched 6.3 px away from where the backward track returns), which the
# check drops as it should; "drops nothing on the unoccluded pair" is a condition on the scene, so the scene is chosen to meet it.
REAL_SEED = OCCLUDER["seed"] + 1
BOX0 = OCCLUDER["box"]                        # y0, y1, x0, x1: the block pasted over the second image of a comparison
BOX1 = (20, 100, 15, 55)                      # a second block elsewhere, for the cam1 image of the GPU test's temporal call


def paste(img, box=BOX0, seed=7):
    """img with a block of foreign texture (uniform noise) pasted over `box`."""
    y0, y1, x0, x1 = box
    out = img.copy()
    out[y0:y1, x0:x1] = np.random.default_rng(seed).integers(0, 256, (y1 - y0, x1 - x0)).astype(np.uint8)
    return out


def depth_in_box(p, box=BOX0):
    """How far the points lie inside the block (positive) or outside it (negative), in pixels."""
    y0, y1, x0, x1 = box
    return np.minimum(np.minimum(p[:, 0] - x0, x1 - 1 - p[:, 0]), np.minimum(p[:, 1] - y0, y1 - 1 - p[:, 1]))


def real_points(cm):
    """The points the real-pair tests track: all cell maxima (cell_maxima records) above the detector threshold."""
    return np.stack([cm["x"], cm["y"]], 1)[cm["score"] > 2560].astype(np.float32)


def real_scene(oracle):
    syn = oracle.Synth(seed=REAL_SEED, width=OCCLUDER["w"], height=OCCLUDER["h"])
    (a0, b0), (a1, b1) = syn.render(REAL_FRAMES[0]), syn.render(REAL_FRAMES[1])
    return syn, a0, b0, a1, b1


def _zeros(n):
    return np.zeros((n, 2), np.float32)


def temporal_verdicts(oracle, a0, a1, pts):
    """Forward a0 -> a1 with the oracle, then the restatement at the defaults: (out0, forward status, status after the gate)."""
    out0, st = oracle.lk_track(a0, a1, pts, pts)
    n = len(pts)
    after = FB.gate(a0, a1, None, FB.TEMPORAL, 1.0, 1.0, 1, pts, out0, _zeros(n), _zeros(n), _zeros(n), st)[4]
    return out0, st, after


def stereo_verdicts(oracle, calib, a, b, pts):
    from msckf_stereo_c_amd.ctypes_types import default_fe_cfg
    out1, m = oracle.stereo_match(calib, default_fe_cfg(), a, b, pts)
    n = len(pts)
    st = (1 | 2 * (np.asarray(m) != 0)).astype(np.uint8)
    after = FB.gate(None, a, b, FB.STEREO, 1.0, 1.0, 0, pts, pts, out1, _zeros(n), _zeros(n), st)[4]
    return out1, st, after


def test_real_pair_at_the_defaults(oracle):
    """Frames 5 and 6 of the occluder scene, the block pasted over the second image of each comparison: at the defaults the
    restatement drops at least half of the forward-surviving points that land 8 px or more inside the block, at most 1 % of those
    8 px or more outside it, and nothing on the unoccluded pair."""
    syn, a0, b0, a1, b1 = real_scene(oracle)
    pts = real_points(oracle.cell_maxima(a0))
    assert len(pts) > 200
    # temporal
    out0, st, after = temporal_verdicts(oracle, a0, paste(a1), pts)
    d = depth_in_box(out0)
    inside, outside = (st != 0) & (d >= 8), (st != 0) & (d <= -8)
    assert inside.sum() >= 20 and outside.sum() >= 100
    print("temporal: inside %d dropped %d, outside %d dropped %d" % (inside.sum(), (after[inside] == 0).sum(), outside.sum(), (after[outside] == 0).sum()))
    assert (after[inside] == 0).sum() * 2 >= inside.sum()
    assert (after[outside] == 0).sum() * 100 <= outside.sum()
    out0, st, after = temporal_verdicts(oracle, a0, a1, pts)
    assert (st != 0).sum() >= 200 and np.array_equal(after, st)
    # stereo
    out1, st, after = stereo_verdicts(oracle, syn.calib, a0, paste(b0), pts)
    d = depth_in_box(out1)
    inside, outside = (st == 3) & (d >= 8), (st == 3) & (d <= -8)
    assert inside.sum() >= 20 and outside.sum() >= 100
    print("stereo: inside %d dropped %d, outside %d dropped %d" % (inside.sum(), (after[inside] == 1).sum(), outside.sum(), (after[outside] == 1).sum()))
    assert (after[inside] == 1).sum() * 2 >= inside.sum()
    assert (after[outside] == 1).sum() * 100 <= outside.sum()
    out1, st, after = stereo_verdicts(oracle, syn.calib, a0, b0, pts)
    assert (st == 3).sum() >= 200 and np.array_equal(after, st)


def gpu_track_images(oracle, do_temporal):
    """(prev0 or None, curr0, curr1) of the GPU test behind a real track: the temporal call sees the block over the current cam0
    image and a second block elsewhere over cam1; the stereo-only call the block over cam1."""
    syn, a0, b0, a1, b1 = real_scene(oracle)
    if do_temporal:
        return a0, paste(a1), paste(b1, BOX1, 8)
    return None, a0, paste(b0)


def gpu_track_points(cm):
    """Every fifth of real_points (about 220, spread over the whole image)."""
    return real_points(cm)[::5]


def test_the_gpu_track_scene_has_both_kinds_of_points(oracle):
    """What test_gpu_fb expects of its real track holds on the oracle: with the check at the defaults each half that runs drops at
    least ten points and keeps at least ten."""
    from msckf_stereo_c_amd.ctypes_types import default_fe_cfg
    syn = real_scene(oracle)[0]
    for do_temporal in (1, 0):
        prev0, curr0, curr1 = gpu_track_images(oracle, do_temporal)
        pts = gpu_track_points(oracle.cell_maxima(prev0 if do_temporal else curr0))
        n = len(pts)
        if do_temporal:
            out0, st = oracle.lk_track(prev0, curr0, pts, pts)
            inb = (out0[:, 0] >= 0) & (out0[:, 0] <= curr0.shape[1] - 1) & (out0[:, 1] >= 0) & (out0[:, 1] <= curr0.shape[0] - 1)
            st = (st != 0) & inb
        else:
            out0, st = pts, np.ones(n, bool)
        k = np.flatnonzero(st)
        out1, status = _zeros(n), np.zeros(n, np.uint8)
        o1, m = oracle.stereo_match(syn.calib, default_fe_cfg(), curr0, curr1, out0[k])
        out1[k], status[k] = o1, 1 | 2 * (np.asarray(m) != 0)
        after = FB.gate(prev0, curr0, curr1, 3, 1.0, 1.0, do_temporal, pts, out0, out1, _zeros(n), _zeros(n), status)[4]
        lost, unmatched = (status != 0) & (after == 0), (status == 3) & (after == 1)
        print("do_temporal %d: %d points, lost %d, unmatched %d, kept %d" % (do_temporal, n, lost.sum(), unmatched.sum(), (after == 3).sum()))
        assert (lost.sum() >= 10) == bool(do_temporal) and unmatched.sum() >= 10 and (after == 3).sum() >= 10


# ------------------------------------------------------------------------------------------ the YAML keys
def test_fb_check_yaml_keys(tmp_path):
    from msckf_stereo_c_amd import build
    from msckf_stereo_c_amd.ctypes_types import FeFbCheck
    build.build_all()
    L = C.CDLL(os.path.join(ROOT, "msckf_stereo_c_amd", "_build", "libmskf_host.so"))
    L.mskfh_load_fb_check.argtypes = [C.c_char_p, C.POINTER(FeFbCheck)]

    def load(path):
        c = FeFbCheck(-1, -1.0, -1.0)
        rc = L.mskfh_load_fb_check(str(path).encode(), C.byref(c))
        return rc, c.mode, c.max_error_temporal, c.max_error_stereo
    stock = os.path.join(ROOT, "config", "app_imgproc.yaml")
    assert load(stock) == (0, 0, 1.0, 1.0)                              # absent means off, with the documented defaults
    text = open(stock).read()
    p = tmp_path / "app_imgproc.yaml"
    for name, mode in (("off", 0), ("temporal", 1), ("stereo", 2), ("both", 3)):
        p.write_text(text + "\nfb_check: %s\nfb_check_max_error_temporal: 0.75\nfb_check_max_error_stereo: 2.5\n" % name)
        assert load(p) == (0, mode, 0.75, 2.5)
    p.write_text(text + "\nfb_check: both\n")
    assert load(p) == (0, 3, 1.0, 1.0)
    p.write_text(text + "\nfb_check: sometimes\n")
    assert load(p)[0] == -1
    for bad in ("far", "-0.5", "64.5", "nan", "inf", "1.0px"):
        p.write_text(text + "\nfb_check: both\nfb_check_max_error_stereo: %s\n" % bad)
        assert load(p)[0] == -1, bad
        p.write_text(text + "\nfb_check_max_error_temporal: %s\n" % bad)
        assert load(p)[0] == -1, bad
    p.write_text(text + "\nfb_check: stereo\nfb_check_max_error_temporal: 0\nfb_check_max_error_stereo: 64\n")
    assert load(p) == (0, 2, 0.0, 64.0)
