"""The coverage conditions of the LK edge cases (tests/lk_cases.py), evaluated on the CPU oracle alone: what the GPU tests
of tests/test_gpu_lk_edges.py feed the kernel reaches the magnitudes, the re-staging and the border gates it is meant to
reach.  The conditions are caps against vacuous inputs, not measurements; a generator that misses one is changed, not the
condition."""
import functools

import numpy as np
import pytest

import lk_cases as C

SIZE_IDS = ["%dx%d" % s for s in C.SIZES]


@functools.lru_cache(maxsize=None)
def _traced(set_name, w, h):
    from oracle import oracle_py as O
    O.build()
    out = []
    for c in C.cases(set_name, w, h, O):
        b, st, tr = O.lk_track_trace(c["A"], c["B"], c["pts"], C.hpred_guess(c["H"], c["pts"]))
        out.append((c, b, st.astype(bool), tr))
    return out


def test_trace_does_not_change_the_track(oracle):
    """The traced entry point returns exactly what lk_track returns."""
    for set_name in ("saturated", "displaced", "border"):
        for c in C.cases(set_name, 129, 71, oracle):
            init = C.hpred_guess(c["H"], c["pts"])
            b0, st0 = oracle.lk_track(c["A"], c["B"], c["pts"], init)
            b1, st1, tr = oracle.lk_track_trace(c["A"], c["B"], c["pts"], init)
            assert np.array_equal(b0.view(np.uint32), b1.view(np.uint32)) and np.array_equal(st0, st1), c["name"]
            assert (tr["lvl"]["solved"][tr["lvl"]["iters"] > 0] == 1).all()
            assert (tr["lvl"]["entered"] >= tr["lvl"]["solved"]).all()


@pytest.mark.parametrize("w,h", C.SIZES, ids=SIZE_IDS)
def test_saturated_set_reaches_the_magnitude_bounds(oracle, w, h):
    """|I| = 4080 (a 0|255 step under a zero sub-pixel offset: (16 * 8160) >> 5), |diff| = 8160 (a black template under a
    white search region) and w11 = -1 on a 255 pixel all occur, and every per-row (lane) and four-row (quad) partial sum
    stays below 2^31: the device keeps both in 32 bits, and sums the sixteen lanes of a window in 64 bits.  The largest observed values are printed (DESIGN.md §3 records
    them next to the derived bound)."""
    runs = _traced("saturated", w, h)
    tr = np.concatenate([r[3] for r in runs])
    ok = np.concatenate([r[2] for r in runs])
    lane, quad, total = tr["lane"].max(0), tr["quad"].max(0), tr["total"][ok].max(0)
    print("%dx%d saturated: max|Ix| %d max|Iy| %d max|diff| %d lane(A11 A12 A22 b1 b2) %s quad %s window total of tracked points %s"
          % (w, h, tr["max_Ix"].max(), tr["max_Iy"].max(), tr["max_diff"].max(), lane.tolist(), quad.tolist(), total.tolist()))
    assert max(tr["max_Ix"].max(), tr["max_Iy"].max()) == 4080
    assert tr["max_diff"].max() == 8160
    assert (tr["w11_neg"] & 2).any()
    assert lane.max() < 2 ** 31 and quad.max() < 2 ** 31
    # the bounds the kernel's comments derive: 15 * 4080^2 per lane for the A terms, 15 * 8160 * 4080 for the b terms
    assert lane[:3].max() <= 15 * 4080 * 4080 and lane[3:].max() <= 15 * 8160 * 4080
    assert quad.max() <= 4 * 15 * 8160 * 4080
    # the whole-window sums of tracked points pass 2^31, in an A term and in a b term: only the 64-bit half of the
    # device's row reduction keeps them (a 32-bit sum would wrap), and at least ten tracked points have such a window
    assert total[:3].max() >= 2 ** 31 and total[3:].max() >= 2 ** 31
    assert int((tr["total"][ok][:, :3].max(1) >= 2 ** 31).sum()) >= 10 and int((tr["total"][ok][:, 3:].max(1) >= 2 ** 31).sum()) >= 10


@pytest.mark.parametrize("set_name", sorted(C.CASE_SETS))
@pytest.mark.parametrize("w,h", C.SIZES, ids=SIZE_IDS)
def test_at_least_half_of_the_in_image_points_are_tracked(oracle, set_name, w, h):
    """An all-lost set proves nothing: per case set and size at least half of the in-image points have status 1."""
    n_in = n_ok = 0
    for c, _, ok, _ in _traced(set_name, w, h):
        inside = C.in_image(c["pts"], w, h)
        n_in += int(inside.sum())
        n_ok += int((ok & inside).sum())
    print("%dx%d %s: %d of %d in-image points tracked" % (w, h, set_name, n_ok, n_in))
    assert 2 * n_ok >= n_in


@pytest.mark.parametrize("w,h", C.SIZES, ids=SIZE_IDS)
def test_displaced_set_forces_restaging(oracle, w, h):
    """At least 50 surviving points whose search window must leave the staged region, at least 10 in each of +x, -x, +y,
    -y, at least 10 at a level other than the coarsest (the reference produces them: a window that straddles two
    differently moved regions settles only at the finer levels), and at least 10 wavefront groups (pt // 4) that mix
    forced and unforced points."""
    n_dir, n_fine, n_any, n_mixed = np.zeros(4, int), 0, 0, 0
    for c, _, ok, tr in _traced("displaced", w, h):
        dirs = C.forced_restage(tr)
        any_level = np.zeros((len(ok), 4), bool)
        for k, d in enumerate(dirs):
            n_dir[k] += int((d.any(1) & ok).sum())
            any_level |= d
        forced = any_level.any(1) & ok
        n_any += int(forced.sum())
        n_fine += int((any_level[:, :3].any(1) & ok).sum())
        n4 = len(ok) // 4 * 4
        g = forced[:n4].reshape(-1, 4)
        n_mixed += int((g.any(1) & ~g.all(1)).sum())
    print("%dx%d displaced: forced %d, +x -x +y -y %s, below the coarsest level %d, mixed groups %d" % (w, h, n_any, n_dir.tolist(), n_fine, n_mixed))
    assert n_any >= 50
    assert (n_dir >= 10).all()
    assert n_fine >= 10
    assert n_mixed >= 10


@pytest.mark.parametrize("w,h", C.SIZES, ids=SIZE_IDS)
def test_border_lattice_hits_every_gate_value(oracle, w, h):
    """Every listed template corner value (-16, -15, -14, -1, 0, n_l - 16, n_l - 15, n_l - 2, n_l - 1, n_l) occurs at every level on every
    side, the guess lattice of the Hpred cases is the same lattice, and every side has tracked and lost points.
    (A point cannot be outside a coarse level's gate and inside level 0's: the gates nest.  The reverse occurs.)"""
    runs = {r[0]["name"]: r for r in _traced("border", w, h)}
    c, _, ok, tr = runs["border_template"]
    pts, side = C.border_points(w, h)
    assert np.array_equal(pts, c["pts"])
    sizes = C.level_sizes(w, h)
    for l in range(4):
        ipx, ipy = tr["lvl"]["ipx"][:, l], tr["lvl"]["ipy"][:, l]
        for (axis, got, n_l, lo, hi) in (("x", ipx, sizes[l][0], 0, 1), ("y", ipy, sizes[l][1], 2, 3)):
            for (v, high) in C.border_values(n_l):
                hit = (got == v) & (side == (hi if high else lo))
                assert hit.any(), (axis, l, v, "side")
                assert ((got == v) & (side == 4)).any(), (axis, l, v, "corner")
                # the gate itself: -16 and n_l are outside, their neighbours inside
                assert (tr["lvl"]["entered"][hit, l] == (0 if v in (-16, n_l) else 1)).all(), (axis, l, v)
    in_coarse_out_fine = (tr["lvl"]["entered"][:, 3] == 1) & (tr["lvl"]["entered"][:, 0] == 0)
    assert in_coarse_out_fine.any()
    assert not ((tr["lvl"]["entered"][:, 3] == 0) & (tr["lvl"]["entered"][:, 0] == 1)).any()
    for s in range(5):
        assert ok[side == s].any() and (~ok[side == s]).any(), s
    for name in ("left", "right", "up", "down"):
        c, _, ok, tr = runs["border_guess_" + name]
        guess = C.hpred_guess(c["H"], c["pts"])
        assert np.array_equal(guess, pts), name           # the translation lands on the lattice exactly
        assert ok.any() and (~ok).any(), name
        # where level 3 iterated, its first search corner is the lattice value
        ran = tr["lvl"]["iters"][:, 3] > 0
        want = np.floor(guess[:, 0].astype(np.float64) / 8 - 7)
        assert ran.any() and np.array_equal(tr["lvl"]["inx0"][ran, 3], want[ran].astype(np.int64))
