"""The named edge cases of the front-end's bookkeeping (csrc/hip/fe_book.h), on the CPU.

tests/cpp/fe_book_device_cases.cpp runs every case through fe_book1 / fe_book2 of the header's host branch, beside ref_frame
(the std::map / std::stable_sort restatement of image_processor.cpp in tests/cpp/fe_book_scenarios.h), and reports a census
per frame.  Here: every case equals ref_frame, never overflows, its descriptor passes the self-check the GPU test runs before
every launch, and its census shows that the case reaches the edge it is named for - which is what keeps the comparison of
k_fe_book with these host runs (tests/test_gpu_fe_book.py) from being vacuous.

test_host_item_order: the host runs the items of a phase (FB_FOR) in ascending order; built with FB_HOST_ORDER = 1
(descending) and 2 (odd indices descending, then even ascending) the same source must leave byte-identical arenas after
fe_book1 and after fe_book2 in every frame of every case, and fe_book_test must print the same summary line.  An item that
reads what another item of its own phase writes, or an output that depends on the slot order of an FB_INC list, fails here.
"""
import subprocess

import numpy as np
import pytest

import fe_book_cases as F

KiB = 1024
DRAWS = 2 * 2 * 7      # a frame whose two RANSAC calls both form hypotheses: 2 cameras x 7 iterations x 2 numbers


def _all(frames, cond):
    return all(cond(c) for c in frames)


def _count_case(n):
    order = [0, 1, 63, 64, 65, 255, 256, 257, 511, 512, 513]
    k = order.index(n)
    below = [order[k - j] if k >= j else 0 for j in (1, 2, 3)]

    def check(fr):
        # frame 0 has n_prev = n and tracks the next smaller count, which is frame 1's n_prev, and so on; the last two refill
        assert fr[0]["n_prev"] == n and fr[0]["n_tracked"] == below[0]
        assert fr[1]["n_prev"] == below[0] and fr[1]["n_tracked"] == below[1]
        assert fr[2]["n_prev"] == below[1] and fr[2]["n_tracked"] == below[2]
        assert fr[2]["n_new"] > 0 and fr[3]["n_prev"] > 256 and fr[3]["max_tracked_cell"] > 6 and fr[3]["max_curr_cell"] == 6
    return check


def _ransac_n_match(n):
    def check(fr):
        c = fr[0]
        assert c["n_prev"] == 300 and c["after_tracking"] == 300 and c["after_matching"] == n
        if n < 3:           # fewer than 3 pairs: nobody is an inlier and nothing is drawn
            assert c["after_ransac"] == 0 and c["draws"] == 0
        else:
            assert c["draws"] == DRAWS and c["after_ransac"] >= 0.9 * n and c["in0"] >= c["after_ransac"] <= c["in1"]
        assert fr[1]["n_prev"] > 256 and fr[1]["draws"] == DRAWS
    return check


def _bounds_16_16(fr):
    assert _all(fr, lambda c: c["max_det_cell"] > 16)                       # the sieve cuts to 16
    assert fr[0]["n_cand"] == 20 * 16 and _all(fr[1:], lambda c: c["max_curr_cell"] == 16)
    assert fr[3]["max_tracked_cell"] > 256                                  # every survivor in one cell, pruned to 16


def _bounds_0_0(fr):
    assert fr[0]["n_prev"] == 12 and fr[0]["n_tracked"] == 8
    assert _all(fr, lambda c: c["n_det"] > 0 and c["n_cand"] == 0 and c["n_new"] == 0 and c["n_curr"] == 0)


def _bounds_0_3(fr):
    assert _all(fr, lambda c: c["n_det"] > 0 and c["n_cand"] == 0 and c["n_new"] == 0 and c["n_tracked"] == 8)
    assert fr[3]["max_tracked_cell"] == 8 and fr[3]["n_curr"] == 3


def _bounds_1_16(fr):
    assert fr[0]["n_cand"] == 20 * 16 and fr[0]["n_new"] == 20              # 16 candidates a cell, one vacancy a cell
    assert fr[3]["max_tracked_cell"] > 16 and fr[3]["max_curr_cell"] == 16


def _crowded(fr):
    c = fr[0]
    assert c["n_tracked"] == 300 and c["max_tracked_cell"] == 300 and c["max_curr_cell"] == 16 == c["grid_max"]
    assert c["n_curr"] == 16 + c["n_new"]
    assert fr[2]["max_tracked_cell"] == fr[2]["n_tracked"] > 64


def _ties(fr):
    assert _all(fr, lambda c: c["score_lo"] == c["score_hi"] > 0 and c["n_det"] > 1000 and c["max_det_cell"] > c["grid_max"])
    assert _all(fr, lambda c: c["n_cand"] == 80 and 0 < c["n_new"] < 60)     # some stereo matches fail: ranks among tied survivors


def _det_no_key(fr):
    assert _all(fr, lambda c: c["keys"] == 0 and c["n_det"] == 0 and c["n_cand"] == 0 and c["n_new"] == 0 and c["n_tracked"] > 0)


def _det_every_cell(fr):
    assert _all(fr, lambda c: c["keys"] == 1410 and c["n_det"] > 1000)
    assert fr[2]["n_tracked"] > 0


def _det_occupied(fr):
    assert _all(fr[:2], lambda c: c["keys"] == 1410 and c["n_tracked"] == 1410 and c["n_det"] == 0 and c["n_cand"] == 0)
    assert fr[2]["max_tracked_cell"] > 16 == fr[2]["max_curr_cell"]


def _det_half_stale(fr):
    assert _all(fr, lambda c: 600 < c["keys"] < 800 and 0 < c["n_det"] <= c["keys"])


def _cand_all_fail(fr):
    assert _all(fr, lambda c: c["n_cand"] == 80 and c["n_new"] == 0 and c["n_curr"] == c["n_tracked"])


def _cand_all_pass(fr):
    assert _all(fr, lambda c: c["n_cand"] == 80 and c["n_curr"] == 60 and c["n_new"] == 60 - c["n_tracked"])


def _cand_last(fr):
    assert _all(fr, lambda c: c["n_cand"] == 80 and c["cells_with_cand"] == 20 and c["n_new"] == 20)


def _q7(fr):
    assert _all(fr[1:3], lambda c: c["max_code"] >= c["n_cells"] and c["n_tracked"] > 0)
    assert fr[3]["n_prev"] > 64


def _ransac_gate(fr):
    for c in (fr[0], fr[2]):
        assert c["after_matching"] == 50 and c["after_ransac"] == 0 and c["draws"] == 0 and c["in0"] == 0 == c["in1"]


def _ransac_rotation(fr):
    assert _all(fr, lambda c: c["after_matching"] >= 300 and c["draws"] == 0 and c["after_ransac"] >= 0.9 * c["after_matching"])


def _ransac_none(fr):
    c = fr[0]
    assert c["after_matching"] == 120 and c["draws"] == DRAWS and c["in0"] == 0 == c["in1"] and c["after_ransac"] == 0
    assert fr[2]["draws"] == DRAWS and fr[2]["after_ransac"] == 0


def _ransac_clean(fr):
    assert _all(fr, lambda c: c["after_matching"] >= 300 and c["draws"] == DRAWS and c["after_ransac"] >= 0.9 * c["after_matching"])


def _ransac_cam1(fr):
    c = fr[0]
    assert c["draws"] == DRAWS and c["in0"] == c["after_matching"] == 300 and c["in1"] == c["after_ransac"] < 250


def _lds(fr):
    assert _all(fr, lambda c: c["n_det"] > 2000 and c["max_det_cell"] > 16)
    assert fr[0]["n_cand"] == 120 * 16 and fr[1]["max_tracked_cell"] > 16 == fr[1]["max_curr_cell"] and fr[2]["n_prev"] > 512


CENSUS = {"grid_16_16": _bounds_16_16, "grid_0_0": _bounds_0_0, "grid_0_3": _bounds_0_3, "grid_1_16": _bounds_1_16,
          "crowded_equal_lifetimes": _crowded, "crowded_tied_lifetimes": _crowded, "ties_q4_off": _ties, "ties_q4_on": _ties,
          "det_no_key": _det_no_key, "det_every_cell": _det_every_cell, "det_every_cell_occupied": _det_occupied, "det_half_stale": _det_half_stale,
          "cand_all_fail": _cand_all_fail, "cand_all_pass": _cand_all_pass, "cand_last_of_cell": _cand_last,
          "q7_333x251_4x5": _q7, "q7_333x251_3x7": _q7, "ransac_gate_leaves_2": _ransac_gate, "ransac_pure_rotation": _ransac_rotation,
          "ransac_no_hypothesis": _ransac_none, "ransac_clean_translation": _ransac_clean, "ransac_cam1_rejects": _ransac_cam1, "lds_over_64k": _lds}
CENSUS.update({"n_prev_%d" % n: _count_case(n) for n in (0, 1, 63, 64, 65, 255, 256, 257, 511, 512, 513)})
CENSUS.update({"ransac_n_match_%d" % n: _ransac_n_match(n) for n in (0, 1, 2, 3, 64, 257)})

SETS = ["counts", "bounds", "crowded", "ties", "detector", "candidates", "q7", "ransac", "lds", "random0", "random1", "random2", "random3"]


def test_case_sets_are_the_named_ones():
    lib = F.lib()
    assert lib.sets == SETS
    named = [n for _, n in lib.cases if not n.startswith("random_")]
    assert sorted(named) == sorted(CENSUS)
    assert len(lib.cases) - len(named) == 40


@pytest.mark.parametrize("case_set", SETS)
def test_cases_equal_reference_flow_and_reach_their_edge(case_set):
    lib = F.lib()
    grid_max, alive = set(), 0
    for i in lib.of_set(case_set):
        r = lib.run(i)
        assert not r.error, (r.name, r.error)                               # == ref_frame, frame after frame
        assert 3 <= r.n_frames <= 8 and len(r.census) == r.n_frames
        print(r.name, "arena %d B, scratch %d B" % (r.size, r.scratch_bytes))
        for f, c in enumerate(r.census):
            print("   frame %d: %s" % (f, " ".join("%s=%d" % kv for kv in c.items())))
            assert c["overflow"] == 0 and c["nan_words"] == 0, (r.name, f)
            assert c["n_prev"] == c["before"] and c["n_curr"] <= c["n_tracked"] + c["n_new"], (r.name, f)
        for f in range(r.n_frames):
            for base in (0x1000, 0x7F0000000000):                           # any base: a low one and one like a device address
                assert r.check_desc(f, r.desc(f, base), base, r.size) is None, (r.name, f)
        # the self-check is not vacuous: an arena one 256-byte region short, a base off by one region, a budget below the scratch
        d = r.desc(0, 0x1000)
        assert r.check_desc(0, d, 0x1000, r.size - 256) is not None
        assert r.check_desc(0, d, 0x1100, r.size) is not None
        assert r.check_desc(0, d, 0x1000, r.size, lds_budget=r.scratch_bytes - 4) is not None
        assert r.scratch_bytes <= 150 * KiB
        if r.name in CENSUS:
            CENSUS[r.name](r.census)
            if case_set == "lds":
                assert 64 * KiB < r.scratch_bytes < 150 * KiB
            else:
                assert r.scratch_bytes <= 64 * KiB
        else:
            grid_max.add(r.census[0]["grid_max"])
            alive += 1 if any(c["n_tracked"] > 64 for c in r.census) else 0
        r.close()
    if case_set.startswith("random"):
        # the widened draw spreads, and most trials have features to track (grid_min = 0 never creates one)
        assert len(grid_max) >= 4 and alive >= 5, (grid_max, alive)


def test_random_cases_reach_both_short_list_bounds():
    lib = F.lib()
    gm = []
    for i in range(len(lib.cases)):
        if lib.cases[i][1].startswith("random_"):
            r = lib.run(i)
            gm.append(r.census[0]["grid_max"])
            r.close()
    assert min(gm) <= 2 and max(gm) == 16 and len(gm) == 40, gm


def test_host_item_order():
    base = subprocess.check_output([F.build_program(0), "400"], text=True)
    assert "device logic == reference flow" in base
    libs = [F.lib(0), F.lib(1), F.lib(2)]
    for order in (1, 2):
        assert subprocess.check_output([F.build_program(order), "400"], text=True) == base, order
    for i, (_, name) in enumerate(libs[0].cases):
        runs = [lib.run(i) for lib in libs]
        for r in runs:
            assert not r.error, (name, r.error)
        assert runs[0].n_frames == runs[1].n_frames == runs[2].n_frames
        for f in range(runs[0].n_frames):
            for which in (1, 3):
                want = runs[0].snapshot(f, which)
                for order in (1, 2):
                    diff = runs[0].where(runs[order].snapshot(f, which), want)
                    assert diff is None, "%s frame %d after fe_book%d, FB_HOST_ORDER %d: %s" % (name, f, 1 + which // 2, order, diff)
        for r in runs:
            r.close()
