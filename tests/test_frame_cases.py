"""The conditions on the inputs of tests/test_gpu_frame_counts.py, shown without a GPU: from k_track4's walk restated in Python
(frame_cases.trips) that the table of (count, launch) pairs holds every shape of the walk it is meant to hold, and from the CPU
oracle alone that the points and the frame sequence reach what they are meant to reach."""
import numpy as np
import pytest

import frame_cases as F
from msckf_stereo_c_amd.ctypes_types import default_ekf_cfg


def _shape(count, launch):
    t = F.trips(count, F.max_pts(count, launch))
    groups = (count + 3) // 4
    return dict(blocks=len(t), groups=groups, trips=[len(x) for x in t], partial_last=count % 4 != 0)


def test_the_walk_restated_takes_every_point_group_once():
    """Whatever the launch is cut for (nothing is launched at max_pts = 0, which only a count of 0 asks for), the blocks of a
    stream take the groups 0 .. ceil(count / 4) - 1 exactly once between them, in ascending order within a block."""
    for count, launch in F.table():
        m = F.max_pts(count, launch)
        t = F.trips(count, m)
        if m == 0:
            assert count == 0 and t == []
            continue
        assert len(t) == (m + 3) // 4
        assert sorted(g for mine in t for g in mine) == list(range((count + 3) // 4)), (count, launch)
        assert all(mine == sorted(mine) for mine in t)


def test_the_table_holds_the_named_shapes():
    table = F.table()
    assert len(table) == len(F.COUNTS) * len(F.LAUNCHES) == 50
    for pair in F.NAMED.values():
        assert pair in table
    z = _shape(*F.NAMED["zero_trips"])
    assert z["blocks"] >= 1 and sum(z["trips"]) == 0                                     # blocks are launched and do nothing
    o = _shape(*F.NAMED["one_trip_partial_last_group"])
    assert o["trips"] == [1] * o["blocks"] and o["groups"] == o["blocks"] and o["partial_last"]
    assert max(_shape(*F.NAMED["three_or_more_trips"])["trips"]) >= 3
    m = _shape(*F.NAMED["more_blocks_than_groups"])
    assert m["blocks"] > m["groups"] >= 1 and m["trips"].count(0) == m["blocks"] - m["groups"]
    # and beyond the named pairs: the launch below, equal to and above the count, for counts that are a multiple of 4, one more
    # and one less
    shapes = {(c, l): _shape(c, l) for c, l in table}
    for rem in (0, 1, 3):
        for rel in (-1, 0, 1):
            assert any(c % 4 == rem and c > 0 and np.sign(F.max_pts(c, l) - c) == rel for c, l in table), (rem, rel)
    assert max(max(s["trips"], default=0) for s in shapes.values()) == 65                # 257 points through one block
    # a block whose trips end on a partly filled group after full ones: the staging of the trip before it is reused
    assert any(s["partial_last"] and s["trips"] and s["trips"][(s["groups"] - 1) % s["blocks"]] >= 2 for s in shapes.values())


def test_the_batch_launch_reaches_two_rounds_and_the_early_exit():
    """Nine descriptors cut for 8 points: 32 blocks; the streams 0 .. 7 and 8 take the blocks of two rounds of the XCD mapping,
    14 blocks belong to no stream and return at once, a stream without points shares the launch with busy ones."""
    n, gps = len(F.BATCH_COUNTS), F.groups_per_stream(F.BATCH_LAUNCH)
    bm = F.block_map(F.launch_blocks(n, F.BATCH_LAUNCH), n, gps)
    assert len(bm) == 32 and bm.count(None) == 14
    assert sorted(x for x in bm if x is not None) == [(si, gi) for si in range(n) for gi in range(gps)]
    assert all(x is None or x[0] % 8 == b % 8 for b, x in enumerate(bm))                  # a stream's blocks are congruent mod 8
    assert {x[0] // 8 for x in bm if x is not None} == {0, 1}
    assert F.BATCH_COUNTS == [0, 257, 1, 33, 4, 64, 5, 32, 3]
    # the zero-count stream's blocks lie between those of busy streams, and share their residue mod 8 with the last stream's
    z = F.BATCH_COUNTS.index(0)
    assert [b for b, x in enumerate(bm) if x is not None and x[0] == z] == [0, 8] and bm[16] == (8, 0) and F.BATCH_COUNTS[8] > 0
    assert max(len(t) for c in F.BATCH_COUNTS for t in F.trips(c, F.BATCH_LAUNCH)) >= 3


def test_the_direct_points_survive_and_get_lost(oracle):
    """Floors on the oracle alone: every direct case of 31 points or more ends with at least 16 points of status 3, and the
    regions1 cases also lose at least 4 points in the temporal half."""
    cases = F.direct_cases(oracle)
    assert sorted(cases) == ["plain", "regions1"]
    for name, c in cases.items():
        assert c["B"].shape == (F.H, F.W) and len(c["pts"]) == 1334 >= max(F.COUNTS)
        full = F.oracle_status(oracle, name, True)
        assert int((full & 1).sum()) == {"plain": 1334, "regions1": 1031}[name]
        assert int((full[:64] & 1).sum()) == {"plain": 64, "regions1": 48}[name]
        for do_temporal in (True, False):
            st = F.oracle_status(oracle, name, do_temporal)
            for count in F.COUNTS:
                if count >= 31:
                    assert int((st[:count] == 3).sum()) >= 16, (name, do_temporal, count)
                    if name == "regions1" and do_temporal:
                        assert int((st[:count] == 0).sum()) >= 4, (name, count)


def test_estimate_restated():
    """mskf_fe_frame_batch_begin: cand_cap / 2 after set_grid, else min(cand_cap, last + last / 2 + 32); the largest stream of the
    batch decides, and the launch is never cut for fewer than 4 points."""
    fe = F.frame_fe_cfg()
    cap = F.cand_cap(fe)
    assert cap == 6 * 8 * 4 + 8
    assert F.estimate([cap], [-1]) == cap // 2
    assert F.estimate([cap], [0]) == 32
    assert F.estimate([cap], [1]) == 33 and F.estimate([cap], [3]) == 36
    assert F.estimate([cap], [150]) == cap                       # 150 + 75 + 32 is cut to the capacity
    assert F.estimate([cap, cap], [0, 100]) == 182 and F.estimate([cap, 88], [0, -1]) == 44
    assert F.estimate([2], [-1]) == 4 and F.estimate([], []) == 4


def test_the_frame_sequence_runs_dry_and_surges(oracle):
    """On the oracle's own front end: the grid is empty on both flat frames and holds 100 features or more on the frame after
    them, which offers more than 64 cell maxima above the threshold: more than two launches' worth of candidates for a launch
    cut from the estimate of a frame without candidates (32), so a block of it takes three trips or more."""
    calib, frames = F.sequence(oracle)
    fe = F.frame_fe_cfg()
    assert len(frames) == F.N_FRAMES == 8 and all(a.shape == (F.FH, F.FW) for a, _ in frames)
    for k in F.FLAT:
        assert (frames[k][0] == 128).all() and (frames[k][1] == 128).all()
    osys = oracle.OracleSystem(calib, fe, default_ekf_cfg())
    n = []
    for k, (a, b) in enumerate(frames):
        osys.stereo(a, b, 0.05 * k)
        n.append(len(osys.dump()[0]))
        if k == 2:
            grid2 = osys.dump()[2].view(np.float32).reshape(-1, 2).copy()
    print("oracle grid sizes", n)
    assert n[3] == 0 and n[4] == 0
    assert min(n[:3]) >= 100 and n[5] >= 100 and min(n[6:]) >= 100
    top = F.maxima_above_threshold(oracle, frames[5][0], fe)
    print("cell maxima above the threshold on frame 5:", len(top))
    assert len(top) >= 65
    est = F.estimate([F.cand_cap(fe)], [0])
    assert est == 32 and max(len(t) for t in F.trips(65, est)) >= 3
    assert len(F.maxima_above_threshold(oracle, frames[3][0], fe)) == 0
    # the drought's first frame still has tracks to lose: the previous grid is tracked into the flat image and nothing matches
    ref = F.track_reference(oracle, calib, fe, frames[2][0], frames[3][0], frames[3][1], grid2)
    print("frame 2's grid into the flat frame 3: before / after tracking / after matching", ref["before_tracking"], ref["after_tracking"], ref["after_matching"])
    assert ref["before_tracking"] == n[2] and ref["after_tracking"] > 50 and ref["after_matching"] == 0
    ref = F.track_reference(oracle, calib, fe, frames[3][0], frames[4][0], frames[4][1], np.zeros((0, 2), np.float32))
    assert (ref["before_tracking"], ref["after_tracking"], ref["after_matching"]) == (0, 0, 0)


@pytest.mark.parametrize("n", [0, 1, 30])
def test_ransac_draws_do_not_depend_on_the_counter(oracle, n):
    """oracle.two_point_ransac draws the same number of samples whatever the draw counter starts at, across 2^32 too: the number
    is set by the success probability (and the early exits), not by the counter; the markers may differ, the increment not."""
    calib, frames = F.sequence(oracle)
    fe = F.frame_fe_cfg(compat=0)
    top = F.maxima_above_threshold(oracle, frames[0][0], fe)[:n]
    p1 = np.stack([top["x"], top["y"]], 1).astype(np.float32) if n else np.zeros((0, 2), np.float32)
    # a flow of a few pixels (a mean flow below one pixel takes the branch that draws nothing) with a little scatter
    p2 = p1 + np.float32([2.5, -1.25]) + np.random.default_rng(n).uniform(-0.3, 0.3, p1.shape).astype(np.float32)
    inc = []
    for start in (0, 7, 2 ** 32 - 5, 2 ** 32 + 11):
        _, after = oracle.two_point_ransac(calib, fe, 0, p1, p2, np.eye(3), draws=start)
        inc.append(after - start)
    print("points", n, "draws", inc)
    assert len(set(inc)) == 1 and inc[0] >= 0
    if n == 30:
        assert inc[0] > 0
