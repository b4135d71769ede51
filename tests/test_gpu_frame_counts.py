"""The device frame's two k_track4 launches at their count edges ("The frame's track launches at their count edges").

a. k_track4 launched directly (fe_launch_track) with the point count on the device (n_pts_dev), over the table of
   tests/frame_cases.py: counts 0 .. 257 against launches cut for 4, 8, 32, the count and the count + 40 points, so that a block
   takes no, one or many point groups and reuses its LDS staging from trip to trip.  The descriptor is the stream's own
   (fe_stream_desc: pyramids, camera models, R01, E, epi_thresh as the ABI stages them); the points, the five outputs and the
   count word lie in one buffer of 0xA5 bytes with 64-byte guards between them, which is compared whole: the first `count`
   entries are bitwise those of mskf_fe_track on the same points and pass the oracle check of tests/lk_cases.py, every other
   byte is untouched.  n_pts is set to count + 1000 (ignored when n_pts_dev is set); every array has count + 1000 entries, so a
   kernel that read it would change poison, not leave the buffer.
b. Whole frames through mskf_fe_frame_batch_begin / _end over a sequence with a drought (two flat frames) and a surge (about 190
   candidates against a launch cut for 32): every exported feature against the oracle, and bitwise independence of the estimate
   a frame was launched with, of the neighbours in its batch, and of where the state came from (mskf_fe_set_grid round trip).
c. The two 64-bit counters (next_feature_id, ransac_draws) across 2^32.

tests/test_frame_cases.py shows without a GPU that these inputs reach what they are meant to reach.  Every bar is bitwise
equality.  The descriptor self-check runs before every direct launch; after a HIP error no test of the module launches anything."""
import ctypes as C

import numpy as np
import pytest

import frame_cases as F
import lk_cases as LC
from msckf_stereo_c_amd import capi
from msckf_stereo_c_amd.ctypes_types import default_ekf_cfg, default_fe_cfg
from test_gpu_detector_edges import FeStreamDev

from hip_runtime import Hip

pytestmark = pytest.mark.gpu

GUARD = 64
OUTS = ("out0", "out1", "und0", "und1", "status")
ARRAYS = (("in_pts", 8),) + tuple((k, 1 if k == "status" else 8) for k in OUTS)
_HIP_ERRORS = []        # after a HIP error no test of this module launches anything
_FRAME_KEYS = ("id", "lifetime", "cam0", "cam1", "und0", "und1")
_FRAME_COUNTS = ("n", "before_tracking", "after_tracking", "after_matching", "after_ransac", "n_candidates", "n_new", "next_feature_id", "ransac_draws")


# ------------------------------------------------------------------------------------------ a. direct launches
@pytest.fixture(scope="module")
def direct(gpu_ctx, oracle):
    """One stream per image pair of the direct launches (prev cam0 = A, curr cam0 = B, curr cam1 = B1)."""
    calib, fe = oracle.euroc_calib(F.W, F.H), default_fe_cfg()
    out = {}
    for name, c in F.direct_cases(oracle).items():
        s = capi.Stream(gpu_ctx, calib, fe, default_ekf_cfg())
        s.push_stereo(c["A"], c["A"])
        s.swap()
        s.push_stereo(c["B"], c["B1"])
        out[name] = (s, c)
    yield dict(streams=out, calib=calib, fe=fe, ref={})
    for s, _ in out.values():
        s.close()


def _host_count(direct, name, count, do_temporal):
    """mskf_fe_track (host count, one trip, the launch equal to the count) on the first `count` points: computed once."""
    key = (name, count, do_temporal)
    if key not in direct["ref"]:
        s, c = direct["streams"][name]
        direct["ref"][key] = s.track(c["pts"][:count], do_temporal=do_temporal, Hpred=c["H"])
    return direct["ref"][key]


def _layout(specs):
    offs, total = [], GUARD
    for _, count, _ in specs:
        o = {}
        for name, size in ARRAYS:
            o[name] = total
            total += (size * (count + F.SLACK) + 63) // 64 * 64 + GUARD
        o["count"] = total
        total += 64 + GUARD
        offs.append(o)
    return offs, total


def _self_check(hip, desc, specs, offs, d_buf, total, cases):
    """Before the launch: every array a descriptor points at lies inside the buffer with at least count (in fact count + SLACK)
    entries and a guard behind it, no two overlap, the pyramids are the stream's and of the case's size, and the count word on
    the device is what was written."""
    spans = []
    for d, (name, count, _), o in zip(desc, specs, offs):
        for field, size in ARRAYS:
            p = getattr(d, field)
            assert p is not None and p == d_buf + o[field], (name, field)
            assert count + F.SLACK >= count >= 0 and p % size == 0 and p + size * (count + F.SLACK) + GUARD <= d_buf + total, (name, field)
            spans.append((p, p + size * (count + F.SLACK)))
        assert d.n_pts_dev == d_buf + o["count"] and d.n_pts_dev % 4 == 0 and d.n_pts_dev + 4 + GUARD <= d_buf + total
        spans.append((d.n_pts_dev, d.n_pts_dev + 4))
        assert hip.get(d.n_pts_dev, 4).view(np.int32)[0] == count, (name, count)
        assert d.n_pts == count + F.SLACK and d.do_temporal in (0, 1)
        h, w = cases[name]["B"].shape
        for pyr in (d.prev0, d.curr0, d.curr1):
            assert [(pyr.w[l], pyr.h[l]) for l in range(4)] == LC.level_sizes(w, h) and all(pyr.lvl[l] for l in range(4))
    spans.sort()
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))


def _direct_launch(gpu_ctx, direct, specs, max_pts):
    """One fe_launch_track over one descriptor per (case name, count, do_temporal), the count on the device.  Returns the buffer
    as it was uploaded, as it came back, and the offsets of every spec's arrays in it."""
    assert not _HIP_ERRORS, "an earlier launch ended with a HIP error: %s" % _HIP_ERRORS
    L = gpu_ctx.L
    L.fe_stream_desc.argtypes = [C.c_void_p, C.POINTER(FeStreamDev)]
    L.fe_stream_desc.restype = C.c_int
    L.fe_launch_track.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    L.fe_launch_track.restype = None
    hip = Hip()
    try:
        offs, total = _layout(specs)
        host = np.full(total, 0xA5, np.uint8)
        for (name, count, _), o in zip(specs, offs):
            pts = direct["streams"][name][1]["pts"][:count]
            host[o["in_pts"]:o["in_pts"] + 8 * count] = np.ascontiguousarray(pts).reshape(-1).view(np.uint8)
            host[o["count"]:o["count"] + 4] = np.array([count], np.int32).view(np.uint8)
        d_buf = hip.alloc(total, False)
        hip.put(d_buf, host)
        desc = (FeStreamDev * len(specs))()
        for d, (name, count, do_temporal), o in zip(desc, specs, offs):
            s, c = direct["streams"][name]
            assert L.fe_stream_desc(s.h, C.byref(d)) == 0
            assert d.n_pts == 0 and not d.n_pts_dev and not d.in_pts and not d.out0 and not d.status      # the point fields are the caller's
            d.n_pts = count + F.SLACK                    # wrong on purpose: ignored when n_pts_dev is set
            d.n_pts_dev = d_buf + o["count"]
            d.do_temporal = int(do_temporal)
            d.Hpred[:] = list(np.asarray(c["H"], np.float64).reshape(-1))
            for field, _ in ARRAYS:
                setattr(d, field, d_buf + o[field])
        _self_check(hip, desc, specs, offs, d_buf, total, {n: direct["streams"][n][1] for n, _, _ in specs})
        raw = np.frombuffer(bytes(desc), np.uint8).copy()
        d_desc = hip.alloc(raw.size, False)
        hip.put(d_desc, raw)
        L.fe_launch_track(d_desc, len(specs), max_pts, gpu_ctx.hip_stream())
        gpu_ctx.sync()
        err = hip.last_error()
        assert err == 0, "hipGetLastError %d after k_track4" % err
        got = hip.get(d_buf, total)
        assert np.array_equal(hip.get(d_desc, raw.size), raw)
    except BaseException as e:
        _HIP_ERRORS.append(repr(e))
        raise
    finally:
        hip.free()
    return host, got, offs


def _expected(direct, host, specs, offs):
    """The uploaded buffer with the first `count` entries of every output replaced by the host-count call's."""
    want = host.copy()
    for (name, count, do_temporal), o in zip(specs, offs):
        ref = _host_count(direct, name, count, do_temporal)
        for k in OUTS:
            a = np.ascontiguousarray(ref[k]).reshape(-1).view(np.uint8)
            assert a.size == (1 if k == "status" else 8) * count
            want[o[k]:o[k] + a.size] = a
    return want


def _outputs(buf, o, count):
    return {k: (buf[o[k]:o[k] + count].copy() if k == "status" else buf[o[k]:o[k] + 8 * count].view(np.float32).reshape(-1, 2).copy()) for k in OUTS}


def _where(got, want, specs, offs):
    """The first differing byte as (spec, array, entry), for the message."""
    bad = np.flatnonzero(got != want)
    if bad.size == 0:
        return None
    b = int(bad[0])
    for spec, o in zip(specs, offs):
        for name, size in ARRAYS + (("count", 4),):
            n = size * (spec[1] + F.SLACK) if name != "count" else 4
            if o[name] <= b < o[name] + n:
                return "%d bytes differ, the first in %s of %s at entry %d (point group %d, row %d of its wavefront)" % (
                    bad.size, name, spec, (b - o[name]) // size, (b - o[name]) // size // 4, (b - o[name]) // size % 4)
    return "%d bytes differ, the first is guard byte %d" % (bad.size, b)


@pytest.mark.parametrize("launch", F.LAUNCHES, ids=[str(l) for l in F.LAUNCHES])
@pytest.mark.parametrize("name", [n for _, n in F.DIRECT])
def test_direct_launch_with_the_count_on_the_device(gpu_ctx, oracle, direct, name, launch):
    """Every count of the table at this launch size, with the temporal half (the case's Hpred) and without it."""
    calib, fe = direct["calib"], direct["fe"]
    c = direct["streams"][name][1]
    n_ok = n_in = 0
    for count in F.COUNTS:
        m = F.max_pts(count, launch)
        for do_temporal in (True, False):
            specs = [(name, count, do_temporal)]
            host, got, offs = _direct_launch(gpu_ctx, direct, specs, m)
            want = _expected(direct, host, specs, offs)
            assert _where(got, want, specs, offs) is None, (count, m, do_temporal, _where(got, want, specs, offs))
            a, b = LC.check_track(_outputs(got, offs[0], count), oracle, calib, fe, F.cut(c, count), do_temporal, (name, count, launch, do_temporal))
            n_ok += a
            n_in += b
        t = F.trips(count, m)
        print("%s count %3d launch %3d: %2d blocks, trips per block at most %2d" % (name, count, m, len(t), max([len(x) for x in t], default=0)))
    print("%s launch %s: %d tracked, %d stereo inliers" % (name, launch, n_ok, n_in))
    assert n_in >= 16 * 2 * sum(1 for x in F.COUNTS if x >= 31)          # the floors of tests/test_frame_cases.py, reached on the device


def test_nine_descriptors_in_one_launch(gpu_ctx, oracle, direct):
    """Counts 0, 257, 1, 33, 4, 64, 5, 32, 3 in one launch cut for 8 points: two rounds of the block -> stream mapping, blocks
    past the last stream, a stream without points among busy ones, mixed images and temporal / stereo-only streams.  Each
    stream's bytes equal those of its own single-descriptor launch and of the host-count call."""
    names = [n for _, n in F.DIRECT]
    specs = [(names[i % 2], count, i % 3 != 2) for i, count in enumerate(F.BATCH_COUNTS)]
    host, got, offs = _direct_launch(gpu_ctx, direct, specs, F.BATCH_LAUNCH)
    want = _expected(direct, host, specs, offs)
    assert _where(got, want, specs, offs) is None, _where(got, want, specs, offs)
    for spec, o in zip(specs, offs):
        h1, g1, o1 = _direct_launch(gpu_ctx, direct, [spec], F.BATCH_LAUNCH)
        lo, hi = o["in_pts"] - GUARD, o["count"] + 64 + GUARD
        assert hi - lo == g1.size and np.array_equal(got[lo:hi], g1), spec
        LC.check_track(_outputs(got, o, spec[1]), oracle, direct["calib"], direct["fe"], F.cut(direct["streams"][spec[0]][1], spec[1]), spec[2], spec)


def test_fe_stream_desc_refuses_what_it_cannot_describe(gpu_ctx, oracle):
    L = gpu_ctx.L
    L.fe_stream_desc.argtypes = [C.c_void_p, C.POINTER(FeStreamDev)]
    L.fe_stream_desc.restype = C.c_int
    s = capi.Stream(gpu_ctx, oracle.euroc_calib(F.W, F.H), default_fe_cfg(), default_ekf_cfg())
    d = FeStreamDev()
    assert L.fe_stream_desc(None, C.byref(d)) == -1 and L.fe_stream_desc(s.h, None) == -1
    assert L.fe_stream_desc(s.h, C.byref(d)) == -1                     # no pair pushed yet
    c = F.direct_cases(oracle)["plain"]
    s.push_stereo(c["B"], c["B1"])
    assert L.fe_stream_desc(s.h, C.byref(d)) == 0 and d.curr0.w[0] == F.W and d.curr1.h[3] == LC.level_sizes(F.W, F.H)[3][1]
    s.swap()
    assert L.fe_stream_desc(s.h, C.byref(d)) == -1                     # the pair has become the previous one
    s.close()


# ------------------------------------------------------------------------------------------ b. frames through the ABI
def _frame(ctx, ss, pairs):
    ctx.frame_batch_begin(ss, pairs, [{} for _ in ss])
    return ctx.frame_batch_end()


def _same_frame(got, want, tag):
    assert [got[k] for k in _FRAME_COUNTS] == [want[k] for k in _FRAME_COUNTS], (tag, [(k, got[k], want[k]) for k in _FRAME_COUNTS if got[k] != want[k]])
    for k in _FRAME_KEYS:
        assert got[k].shape == want[k].shape and got[k].tobytes() == want[k].tobytes(), (tag, k)


def _cfg(kind):
    return F.frame_fe_cfg() if kind == "6x8" else default_fe_cfg()


_LONE = {}


def _lone(oracle, kind="6x8", shift=0):
    """The sequence (rotated by `shift` frames) through one stream alone on a context of its own, after an empty set_grid:
    the frame results, computed once."""
    if (kind, shift) not in _LONE:
        calib, frames = F.sequence(oracle)
        ctx = capi.Context(0)
        try:
            s = capi.Stream(ctx, calib, _cfg(kind), default_ekf_cfg())
            s.set_grid()
            _LONE[(kind, shift)] = [_frame(ctx, [s], [frames[(t + shift) % F.N_FRAMES]])[0] for t in range(F.N_FRAMES)]
            s.close()
        finally:
            ctx.close()
    return _LONE[(kind, shift)]


def _counters(r):
    return [r["after_tracking"], r["after_matching"], r["after_ransac"]]


def _grid(r):
    return {k: r[k] for k in _FRAME_KEYS}


def test_frames_against_the_oracle(gpu_ctx, oracle):
    """Every frame of the sequence: the counters and every exported feature against the oracle run on the previous frame's
    exported cam0 points; the drought gives no candidates, the frame after it more than twice what its launch was cut for.
    A frame whose previous grid is empty leaves the after_* counters as they were (image_processor.cpp:383)."""
    calib, frames = F.sequence(oracle)
    fe = F.frame_fe_cfg()
    res = _lone(oracle)
    cap = F.cand_cap(fe)
    twin = capi.Stream(gpu_ctx, calib, fe, default_ekf_cfg())
    last, next_id = -1, 0
    prev = dict(n=0, cam0=np.zeros((0, 2), np.float32), id=np.zeros(0, np.uint64), lifetime=np.zeros(0, np.int32), after_tracking=0, after_matching=0, after_ransac=0)
    n_old = n_fresh = 0
    for k, r in enumerate(res):
        cam0, cam1 = frames[k]
        est = F.estimate([cap], [last])
        t = max((len(x) for x in F.trips(r["n_candidates"], est)), default=0)
        print("frame %d: n %3d, before / after tracking / after matching %3d %3d %3d, n_candidates %3d against a launch cut for %3d: %d trips, n_new %3d" % (
            k, r["n"], r["before_tracking"], r["after_tracking"], r["after_matching"], r["n_candidates"], est, t, r["n_new"]))
        # the first launch: the previous grid tracked into this frame
        ref = F.track_reference(oracle, calib, fe, frames[k - 1][0], cam0, cam1, prev["cam0"])
        assert r["before_tracking"] == ref["before_tracking"] == prev["n"], k
        want = [ref["after_tracking"], ref["after_matching"]] if prev["n"] else [prev["after_tracking"], prev["after_matching"]]
        assert [r["after_tracking"], r["after_matching"]] == want, k
        assert r["after_ransac"] == r["after_matching"]                                   # (no RANSAC in this configuration)
        old = np.flatnonzero(r["lifetime"] > 1)
        where = {int(i): j for j, i in enumerate(prev["id"])}
        src = np.array([where[int(i)] for i in r["id"][old]], np.int64)
        assert len(set(src.tolist())) == len(src) <= ref["after_matching"]
        assert ref["ok"][src].all() and ref["inl"][src].all(), k
        assert np.array_equal(r["lifetime"][old], prev["lifetime"][src] + 1), k
        for key in ("cam0", "cam1", "und0", "und1"):
            assert LC.same(r[key][old], ref[key][src]), (k, key)
        # the second launch: the new features are cell maxima of this pair, matched and undistorted as the oracle does
        new = np.flatnonzero(r["lifetime"] == 1)
        assert len(old) + len(new) == r["n"] and len(new) == r["n_new"], k
        twin.push_stereo(cam0, cam1)
        m = twin.cell_maxima()
        m = m[m["score"] > fe.fast_threshold * 256]
        maxima = {(float(x), float(y)) for x, y in zip(m["x"], m["y"])}
        assert all((float(x), float(y)) in maxima for x, y in r["cam0"][new]), k
        sref = F.stereo_reference(oracle, calib, fe, cam0, cam1, r["cam0"][new])
        assert sref["inl"].all(), k
        for key in ("cam1", "und0", "und1"):
            assert LC.same(r[key][new], sref[key]), (k, key)
        assert sorted(int(i) for i in r["id"][new]) == list(range(next_id, next_id + r["n_new"])) and r["next_feature_id"] == next_id + r["n_new"], k
        assert r["n_candidates"] <= min(cap, len(m)), k
        n_old += len(old)
        n_fresh += len(new)
        last, next_id, prev = r["n_candidates"], r["next_feature_id"], r
    twin.close()
    # the path was taken: nothing to choose from in the drought, and a surge the launch was not cut for
    assert res[3]["n_candidates"] == 0 and res[4]["n_candidates"] == 0 and res[3]["n"] == 0 and res[4]["n"] == 0
    assert res[3]["before_tracking"] > 100 and res[4]["before_tracking"] == 0
    assert res[5]["n_candidates"] > 2 * F.estimate([cap], [res[4]["n_candidates"]]) == 64
    assert res[5]["n"] >= 100 and n_old > 400 and n_fresh > 200


def test_a_frame_does_not_depend_on_the_estimate_it_was_launched_with(oracle):
    """Stream X reaches frame 5 through the drought: its second launch is cut for 32 points.  Stream Y pushes frame 4 as a frame,
    then takes X's counters with an empty mskf_fe_set_grid, which resets the estimate to cand_cap / 2 = 100.  Frames 5, 6 and 7
    are identical."""
    calib, frames = F.sequence(oracle)
    fe = F.frame_fe_cfg()
    x = _lone(oracle)
    assert F.estimate([F.cand_cap(fe)], [x[4]["n_candidates"]]) == 32 and F.estimate([F.cand_cap(fe)], [-1]) == 100
    ctx = capi.Context(0)
    try:
        y = capi.Stream(ctx, calib, fe, default_ekf_cfg())
        y.set_grid()
        assert _frame(ctx, [y], [frames[4]])[0]["n"] == 0
        y.set_grid(n=0, next_feature_id=x[4]["next_feature_id"], tracking_counters=_counters(x[4]), ransac_draws=x[4]["ransac_draws"])
        for k in (5, 6, 7):
            _same_frame(_frame(ctx, [y], [frames[k]])[0], x[k], k)
        assert x[5]["n_candidates"] > 64 and x[5]["n"] >= 100
        y.close()
    finally:
        ctx.close()


def test_a_frame_does_not_depend_on_its_neighbours(oracle):
    """Three streams run the sequence rotated by 0, 2 and 4 frames in one batch, so that one is in its drought while another
    surges and the launches are cut for the busiest; a fourth has the default grid configuration (other capacities).  Every
    stream equals its run alone."""
    calib, frames = F.sequence(oracle)
    who = [("6x8", 0), ("6x8", 2), ("6x8", 4), ("4x5", 0)]
    alone = [_lone(oracle, kind, shift) for kind, shift in who]
    caps = [F.cand_cap(_cfg(kind)) for kind, _ in who]
    assert len(set(caps)) == 2
    ctx = capi.Context(0)
    try:
        ss = [capi.Stream(ctx, calib, _cfg(kind), default_ekf_cfg()) for kind, _ in who]
        assert ss[0].grid_capacity() != ss[3].grid_capacity()
        for s in ss:
            s.set_grid()
        differs = 0
        last = [-1] * len(who)
        for t in range(F.N_FRAMES):
            got = _frame(ctx, ss, [frames[(t + shift) % F.N_FRAMES] for _, shift in who])
            own = [F.estimate([caps[i]], [last[i]]) for i in range(len(who))]
            differs += sum(1 for e in own if e != F.estimate(caps, last))
            for i, g in enumerate(got):
                _same_frame(g, alone[i][t], (t, who[i]))
            print("step %d: n_candidates %s, launches alone %s, in the batch %d" % (t, [g["n_candidates"] for g in got], own, F.estimate(caps, last)))
            last = [g["n_candidates"] for g in got]
        # a drought beside a surge, and launches that were cut differently than alone
        assert any(alone[1][t]["n_candidates"] == 0 and alone[2][t]["n_candidates"] > 64 for t in range(F.N_FRAMES))
        assert differs >= 4
        for s in ss:
            s.close()
    finally:
        ctx.close()


def test_exported_grid_and_counters_are_the_whole_state(oracle):
    """After frame 6 of the lone run: a fresh stream of a fresh context gets frame 6 as its previous pair (push, swap) and the
    exported grid and counters (mskf_fe_set_grid with n > 0), then runs frame 7: identical to the original's frame 7."""
    calib, frames = F.sequence(oracle)
    x = _lone(oracle)
    assert x[6]["n"] > 100
    ctx = capi.Context(0)
    try:
        z = capi.Stream(ctx, calib, F.frame_fe_cfg(), default_ekf_cfg())
        z.push_stereo(*frames[6])
        z.swap()
        z.set_grid(next_feature_id=x[6]["next_feature_id"], tracking_counters=_counters(x[6]), ransac_draws=x[6]["ransac_draws"], **_grid(x[6]))
        _same_frame(_frame(ctx, [z], [frames[7]])[0], x[7], "frame 7")
        assert x[7]["before_tracking"] == x[6]["n"] and (x[7]["lifetime"] > 1).sum() > 100
        z.close()
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------ c. the counters across 2^32
def _moving(oracle):
    """Frames 0, 2, 4, 6 of the same scene with the camera moving from frame 1 on: the flow between frames is well above the pixel
    below which the RANSAC draws nothing."""
    syn = oracle.Synth(seed=F.SEED, width=F.FW, height=F.FH, n_static=1, n_loop=40)
    return [syn.render(k) for k in (0, 2, 4, 6)]


@pytest.mark.parametrize("which", ["static", "moving"])
def test_counters_across_2_to_the_32(oracle, which):
    """compat = 0: RANSAC on.  Two streams run three frames side by side; then each takes its exported grid back, one with the exported
    counters, one with next_feature_id = 2^32 - 3 and ransac_draws = 2^32 - 5, and both run the next frame (frame 5 of the
    sequence; frame 6 of the moving one).  The ids run on from the start value across 2^32, the draws advance by the same
    number (set by the success probability, not by the counter: tests/test_frame_cases.py), and what does not depend on the
    draws is identical."""
    calib, frames = F.sequence(oracle)
    seq = [frames[0], frames[1], frames[2], frames[5]] if which == "static" else _moving(oracle)
    fe = F.frame_fe_cfg(compat=0)                         # no compatibility flag: the RANSAC runs inside the frame
    ctx = capi.Context(0)
    try:
        ss = [capi.Stream(ctx, calib, fe, default_ekf_cfg()) for _ in range(2)]
        for s in ss:
            s.set_grid()
        for pair in seq[:3]:
            a, b = _frame(ctx, ss, [pair, pair])
            _same_frame(a, b, "side by side")
        assert a["n"] > 50
        starts = [(a["next_feature_id"], a["ransac_draws"]), (2 ** 32 - 3, 2 ** 32 - 5)]
        for s, (nid, draws) in zip(ss, starts):
            s.set_grid(next_feature_id=nid, tracking_counters=_counters(a), ransac_draws=draws, **_grid(a))
        r = _frame(ctx, ss, [seq[3], seq[3]])
        inc = [x["ransac_draws"] - draws for x, (_, draws) in zip(r, starts)]
        print("%s: n_new %s, next_feature_id %s, ransac_draws %s (+%s), after tracking / matching / ransac %s" % (
            which, [x["n_new"] for x in r], [x["next_feature_id"] for x in r], [x["ransac_draws"] for x in r], inc,
            [(x["after_tracking"], x["after_matching"], x["after_ransac"]) for x in r]))
        for x, (nid, _) in zip(r, starts):
            assert x["next_feature_id"] == nid + x["n_new"]
            new = x["lifetime"] == 1
            assert sorted(int(i) for i in x["id"][new]) == list(range(nid, nid + x["n_new"]))
            assert x["n"] > 0 and x["before_tracking"] == a["n"]
        assert r[1]["next_feature_id"] > 2 ** 32 and r[1]["n_new"] >= 4
        assert inc[0] == inc[1] >= 0
        if which == "moving":
            assert inc[0] > 0 and r[1]["ransac_draws"] > 2 ** 32
        for k in ("before_tracking", "after_tracking", "after_matching"):
            assert r[0][k] == r[1][k], k
        for s in ss:
            s.close()
    finally:
        ctx.close()
