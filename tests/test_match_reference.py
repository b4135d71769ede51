"""The descriptor matcher's contract ("Descriptor matching") on the CPU: the hand-made jobs of
tests/match_cases.py give the answers written beside them, a slow double loop over the definition == the numpy restatement
(tests/match_reference.py) on every job, csrc/hip/fe_match.h (the header the kernel and the C ABI run) compiled with g++ == the
restatement on every job with the scanned sets cut in two at every place and merged under the header's rule, and the property
that makes the matcher worth having: it finds a point again in a moved, noisy view."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import brief_reference as BR
import lk_cases as LK
import match_cases as MC
import match_reference as MR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BY_NAME = {c["name"]: c for c in MC.CASES}
FIELDS = ("idx", "nearest", "dist", "second")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("fe_match") / "libfe_match_test.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-shared", "-fPIC", "-I", ROOT, "-o", so,
                           os.path.join(ROOT, "tests", "cpp", "fe_match_test.cpp")])
    L = C.CDLL(so)
    L.fm_match.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_int, C.c_int, C.c_void_p]
    L.fm_match_splits.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_int, C.c_int, C.c_int,
                                  C.c_void_p, C.c_int, C.c_void_p]
    L.fm_merge_of.argtypes = [C.c_void_p] * 3
    L.fm_merge_of.restype = None

    def ptr(a):
        return None if a is None or a.size == 0 else a.ctypes.data

    class H:
        lib = L

        @staticmethod
        def job(c):
            return (ptr(c["query"]), ptr(c["query_valid"]), len(c["query"]), ptr(c["train"]), ptr(c["train_valid"]), len(c["train"]),
                    c["max_distance"], c["ratio"], int(c["cross_check"]))

        @staticmethod
        def match(c, split=0):
            out = np.zeros(len(c["query"]), MR.MATCH)
            out[:] = (-7, -7, 0xEEEE, 0xEEEE)
            n = L.fm_match(*H.job(c), split, ptr(out))
            return out, n

        @staticmethod
        def bad_splits(c, first, last, want, want_n):
            scratch = np.zeros(len(c["query"]), MR.MATCH)
            want = np.ascontiguousarray(want)
            return L.fm_match_splits(*H.job(c), first, last, ptr(want), want_n, ptr(scratch))

        @staticmethod
        def merge(a, b):
            x, y, out = np.array(a, np.uint32), np.array(b, np.uint32), np.zeros(2, np.uint32)
            L.fm_merge_of(x.ctypes.data, y.ctypes.data, out.ctypes.data)
            return tuple(int(v) for v in out)
    return H


_want = {}


def reference(c):
    """match_reference.match of a case, computed once."""
    if c["name"] not in _want:
        m, n = MR.match(**MC.options(c))
        m.setflags(write=False)
        _want[c["name"]] = (m, n)
    return _want[c["name"]]


def _same(got, want, what):
    for k in FIELDS:
        assert np.array_equal(got[0][k], want[0][k]), (what, k, np.flatnonzero(got[0][k] != want[0][k])[:8])
    assert got[1] == want[1], (what, "n_matches")


# ------------------------------------------------------------------------------------------ the cases
def test_cases_cover_what_they_should():
    names = set(BY_NAME)
    for nq in [0, 1, 63, 64, 65, 129]:
        for nt in [0, 1, 2, 63, 64, 65, MR.TILE - 1, MR.TILE, MR.TILE + 1, 2 * MR.TILE + 1]:
            c = BY_NAME["size %dx%d" % (nq, nt)]
            assert (len(c["query"]), len(c["train"])) == (nq, nt)
    assert {"3x65535", "65535x2"} <= names
    assert len(BY_NAME["3x65535"]["train"]) == 65535 == MR.MAX_N and len(BY_NAME["65535x2"]["query"]) == 65535
    sized = [c for c in MC.CASES if c["name"].startswith("size")]
    for key in ("query_valid", "train_valid"):
        assert any(c[key] is not None for c in sized) and any(c[key] is None for c in sized)
        big = [c[key] for c in sized if c[key] is not None and len(c[key]) >= 65]
        assert big and all(v[0] == 0 and v[63] == 0 and v[64] == 0 and v[-1] == 0 and v.any() for v in big)
    assert any(c["cross_check"] for c in sized) and any(not c["cross_check"] for c in sized)
    # the jobs reject some and accept some, and distances are small where a train descriptor descends from the query
    acc = rej = 0
    for c in sized:
        m, n = reference(c)
        acc += n
        rej += int(((m["idx"] < 0) & (m["nearest"] >= 0)).sum())
    assert acc > 500 and rej > 500
    m, _ = reference(BY_NAME["size 129x%d" % (2 * MR.TILE + 1)])
    assert np.median(m["dist"][m["nearest"] >= 0]) <= 12


@pytest.mark.parametrize("name", [c["name"] for c in MC.CASES if c["want"] is not None])
def test_known_answers(name):
    c = BY_NAME[name]
    m, n = reference(c)
    for k, v in c["want"].items():
        assert m[k].tolist() == list(v), (name, k, m[k].tolist())
    assert n == sum(1 for v in c["want"]["idx"] if v >= 0)


def test_float32_ratio_rule_is_what_the_cases_say():
    f = np.float32
    assert f(0.8) * f(5) == f(4) and not f(4) < f(0.8) * f(5)            # the product rounds down to 4.0
    assert float(f(0.8)) > 0.8 and float(f(0.8)) * 5 > 4.0               # the float32 of 0.8 is above 0.8: a double product would accept 4 against 5
    assert f(3) < f(0.8) * f(5) and not f(3) < f(0.75) * f(4)


# ------------------------------------------------------------------------------------------ the definition, slowly
def _popcount(v):
    return bin(v).count("1")


def match_slow(c):
    """The definition as a double loop over Python integers."""
    q = [int.from_bytes(bytes(r), "little") for r in c["query"]]
    t = [int.from_bytes(bytes(r), "little") for r in c["train"]]
    qv = [True] * len(q) if c["query_valid"] is None else [bool(v) for v in c["query_valid"]]
    tv = [True] * len(t) if c["train_valid"] is None else [bool(v) for v in c["train_valid"]]
    ratio = np.float32(c["ratio"])
    bwd = {}

    def backward(j):
        if j not in bwd:
            bwd[j] = min((_popcount(q[i] ^ t[j]), i) for i in range(len(q)) if qv[i])[1]
        return bwd[j]
    out = np.zeros(len(q), MR.MATCH)
    n = 0
    for i in range(len(q)):
        pairs = sorted((_popcount(q[i] ^ t[j]), j) for j in range(len(t)) if tv[j]) if qv[i] else []
        if not pairs:
            out[i] = (-1, -1, MR.NONE, MR.NONE)
            continue
        (dist, nearest), second = pairs[0], (pairs[1][0] if len(pairs) > 1 else MR.NONE)
        ok = dist <= c["max_distance"]
        if ok and ratio != 0 and second != MR.NONE:
            ok = bool(np.float32(dist) < ratio * np.float32(second))
        if ok and c["cross_check"]:
            ok = backward(nearest) == i
        out[i] = (nearest if ok else -1, nearest, dist, second)
        n += ok
    return out, n


def _slow_sorted_is_too_slow(c):
    return len(c["query"]) * len(c["train"]) > 70000


def match_slow_large(c):
    """The same for the two jobs with 65535 descriptors on one side, without sorting every row."""
    q = [int.from_bytes(bytes(r), "little") for r in c["query"]]
    t = [int.from_bytes(bytes(r), "little") for r in c["train"]]
    qv = [True] * len(q) if c["query_valid"] is None else [bool(v) for v in c["query_valid"]]
    tv = [True] * len(t) if c["train_valid"] is None else [bool(v) for v in c["train_valid"]]
    ratio = np.float32(c["ratio"])
    bwd = {}
    out = np.zeros(len(q), MR.MATCH)
    n = 0
    for i in range(len(q)):
        best, second = None, MR.NONE
        if qv[i]:
            for j in range(len(t)):
                if not tv[j]:
                    continue
                d = _popcount(q[i] ^ t[j])
                if best is None or d < best[0]:                   # (j rises: an equal distance does not replace the lower index)
                    best, second = (d, j), (second if best is None else min(second, best[0]))
                else:
                    second = min(second, d)
        if best is None:
            out[i] = (-1, -1, MR.NONE, MR.NONE)
            continue
        dist, nearest = best
        ok = dist <= c["max_distance"]
        if ok and ratio != 0 and second != MR.NONE:
            ok = bool(np.float32(dist) < ratio * np.float32(second))
        if ok and c["cross_check"]:
            if nearest not in bwd:
                bwd[nearest] = min((_popcount(q[k] ^ t[nearest]), k) for k in range(len(q)) if qv[k])[1]
            ok = bwd[nearest] == i
        out[i] = (nearest if ok else -1, nearest, dist, second)
        n += ok
    return out, n


@pytest.mark.parametrize("name", [c["name"] for c in MC.CASES])
def test_reference_equals_definition(name):
    c = BY_NAME[name]
    _same((match_slow_large if _slow_sorted_is_too_slow(c) else match_slow)(c), reference(c), name)


# ------------------------------------------------------------------------------------------ the header against the restatement
def test_header_constants_and_layout(harness):
    out = (C.c_int * 4)()
    assert harness.lib.fm_constants(out) == 4
    assert list(out) == [MR.TILE, MR.MAX_N, MR.NONE, MR.MATCH.itemsize] == [MC.T, 65535, 0xFFFF, 12]
    lay = (C.c_int * 32)()
    n = harness.lib.fm_match_dev_layout(lay, 32)
    assert list(lay[n - 5:n]) == [12] + [MR.MATCH.fields[k][1] for k in FIELDS]


LARGE_SPLITS = [0, 1, 2, 255, 256, 257, 1000, 1001, 32768, 65470, 65533, 65534, 65535]


@pytest.mark.parametrize("name", [c["name"] for c in MC.CASES])
def test_header_equals_restatement_at_every_split(harness, name):
    """The header's host function == numpy, and so is the merge of two parts of every scan cut at 0 .. the larger of nq and nt
    (the backward scan is cut too).  The two jobs with 65535 descriptors are cut at LARGE_SPLITS only: every place would be
    65535 full jobs."""
    c = BY_NAME[name]
    want = reference(c)
    _same(harness.match(c), want, name)
    n = max(len(c["query"]), len(c["train"]))
    if n <= 2 * MR.TILE + 1:
        assert harness.bad_splits(c, 0, n + 1, want[0], want[1]) == 0
    else:
        for s in LARGE_SPLITS:
            _same(harness.match(c, s), want, (name, s))


def test_header_refuses_what_the_abi_refuses(harness):
    c = dict(BY_NAME["size 1x2"])
    for change in (dict(max_distance=-1), dict(max_distance=257), dict(ratio=-0.1), dict(ratio=1.5), dict(ratio=float("nan"))):
        assert harness.match(dict(c, **change))[1] == -1, change


def test_merge_rule(harness):
    """best = the smaller key, second = the smallest of the losing key's distance and the two seconds; the empty part is neutral; the
    order of three parts does not matter."""
    none = (0xFFFFFFFF, 0xFFFF)
    a, b, c = ((3 << 16) | 7, 9), ((3 << 16) | 2, 0xFFFF), ((5 << 16) | 1, 5)
    assert harness.merge(a, b) == harness.merge(b, a) == ((3 << 16) | 2, 3)
    assert harness.merge(a, none) == a and harness.merge(none, a) == a and harness.merge(none, none) == none
    assert harness.merge(a, c) == ((3 << 16) | 7, 5)
    assert harness.merge(harness.merge(a, b), c) == harness.merge(a, harness.merge(b, c)) == harness.merge(harness.merge(c, a), b) == ((3 << 16) | 2, 3)


# ------------------------------------------------------------------------------------------ worth having
# canvas -> correct correspondences of the 126 lattice points with cross-check on: (ratio off, ratio 0.8)
WORTH = {"smooth": (122, 116), "blocks8": (119, 112), "edges": (126, 126)}
N_LATTICE = 126


@pytest.mark.parametrize("name", ["smooth", "blocks8", "edges"])
def test_matcher_finds_a_point_again(name):
    """The three canvases and two views of the descriptor's own "worth having" test: 160 x 120, seed 7, the second view moved by
    (3, -2) with uniform noise of +-4 grey levels, a 9 px lattice 20 px inside.  The numpy matcher with cross-check on, without
    and with ratio 0.8: the number of lattice points whose match is the same point in the other view.  Deterministic; measured on
    the restatement, never on the device."""
    w, h, seed = 160, 120, 7
    canvas = {"smooth": lambda: LK.smooth_canvas(w, h, seed), "blocks8": lambda: LK.block_canvas(w, h, 8, seed), "edges": lambda: LK.edge_canvas(w, h, seed)}[name]()
    A = LK.crop(canvas, w, h)
    noise = np.random.default_rng(seed).integers(-4, 5, (h, w))
    B = (LK.crop(canvas, w, h, 3, -2).astype(np.int64) + noise).clip(0, 255).astype(np.uint8)
    pts = np.array([(x, y) for y in range(20, h - 20, 9) for x in range(20, w - 20, 9)], np.float32)
    assert len(pts) == N_LATTICE
    dA, vA = BR.describe(A, pts)
    dB, vB = BR.describe(B, pts + np.array([3, -2], np.float32))
    got = []
    for ratio in (0.0, 0.8):
        m, n = MR.match(dA, dB, vA, vB, cross_check=True, ratio=ratio)
        correct = int((m["idx"] == np.arange(len(pts))).sum())
        assert correct <= n <= len(pts)
        got.append((correct, n))
    print("matcher %s: correct / accepted of %d: ratio off %d / %d, ratio 0.8 %d / %d" % (name, len(pts), got[0][0], got[0][1], got[1][0], got[1][1]))
    assert (got[0][0], got[1][0]) == WORTH[name]
