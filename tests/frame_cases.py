"""What drives the device frame's two k_track4 launches (mskf_fe_frame_batch_begin) at their count edges, and the CPU oracle's
side of what they must give.

The second launch of a frame does not know its point count: the descriptor's n_pts_dev points at the candidate count
k_fe_book leaves on the device, the grid is cut from an estimate, and a block walks
    for (gq = gi; 4 * gq < n_pts; gq += groups_per_stream)
over the point groups of its stream.  Both launches are cut for the largest stream of the batch.  Here are

  - the table of (count, launch size) pairs for direct launches of k_track4 with the count on the device, and the kernel's
    loop restated (trips), from which tests/test_frame_cases.py shows which shapes of the walk the table contains;
  - the launch-size estimate of mskf_fe_frame_batch_begin restated (estimate);
  - the frame sequence that takes a stream through a drought (two flat frames) into a surge of candidates, and the oracle's
    answer for one frame's tracks (track_reference).

tests/test_frame_cases.py holds the conditions (no GPU); tests/test_gpu_frame_counts.py runs everything on the device.
"""
import numpy as np

import lk_cases as LC

W, H = 376, 240                                        # the direct launches
COUNTS = [0, 1, 3, 4, 5, 31, 32, 33, 64, 257]
LAUNCHES = [4, 8, 32, "count", "count+40"]             # max_pts handed to fe_launch_track
SLACK = 1000                                           # entries every buffer has beyond the count (and n_pts is count + SLACK: ignored)
DIRECT = (("sizes", "plain"), ("displaced", "regions1"))
# (count, launch) pairs of the table that tests/test_frame_cases.py asserts by name
NAMED = {"zero_trips": (0, 4), "one_trip_partial_last_group": (5, 8), "three_or_more_trips": (33, 8),
         "more_blocks_than_groups": (1, 32)}
BATCH_COUNTS = [0, 257, 1, 33, 4, 64, 5, 32, 3]        # one launch of nine descriptors ...
BATCH_LAUNCH = 8                                       # ... cut for 8 points


def max_pts(count, launch):
    return {"count": count, "count+40": count + 40}.get(launch, launch)


def table():
    return [(c, l) for c in COUNTS for l in LAUNCHES]


def groups_per_stream(max_pts_):
    """fe_launch_track: blocks per stream of a launch cut for max_pts points (0: nothing is launched)."""
    return (max_pts_ + 3) // 4 if max_pts_ > 0 else 0


def trips(count, max_pts_):
    """k_track4's walk restated: per block gi of a stream, the point groups gq it takes (one trip of the loop each)."""
    gps = groups_per_stream(max_pts_)
    out = []
    for gi in range(gps):
        mine, gq = [], gi
        while 4 * gq < count:
            mine.append(gq)
            gq += gps
        out.append(mine)
    return out


def block_map(n_blocks, n_streams, gps):
    """k_track4's block -> (stream, group) mapping restated: blocks b and b + 8 go to one stream; None: the block returns."""
    out = []
    for b in range(n_blocks):
        x, qb = b & 7, b >> 3
        si, gi = x + 8 * (qb // gps), qb % gps
        out.append((si, gi) if si < n_streams else None)
    return out


def launch_blocks(n_streams, max_pts_):
    return 8 * ((n_streams + 7) // 8) * groups_per_stream(max_pts_)


_DIRECT = {}


def direct_cases(oracle):
    """name -> case (tests/lk_cases.py) of the two image pairs of the direct launches."""
    if not _DIRECT:
        for set_name, name in DIRECT:
            _DIRECT[name] = [c for c in LC.cases(set_name, W, H, oracle) if c["name"] == name][0]
    return _DIRECT


def cut(c, count):
    """The case with its first `count` points."""
    out = dict(c)
    out["pts"] = np.ascontiguousarray(c["pts"][:count])
    return out


_STATUS = {}


def oracle_status(oracle, name, do_temporal):
    """Status byte (bit 0 tracked, bit 1 stereo inlier) the oracle gives every point of a direct case."""
    from msckf_stereo_c_amd.ctypes_types import default_fe_cfg
    key = (name, bool(do_temporal))
    if key not in _STATUS:
        c = direct_cases(oracle)[name]
        calib, fe = oracle.euroc_calib(W, H), default_fe_cfg()
        pts = c["pts"]
        if do_temporal:
            b, st = oracle.lk_track(c["A"], c["B"], pts, LC.hpred_guess(c["H"], pts))
            ok = st.astype(bool) & LC.in_image(b, W, H)
        else:
            b, ok = pts, np.ones(len(pts), bool)
        status = np.zeros(len(pts), np.uint8)
        if ok.any():
            _, inl = oracle.stereo_match(calib, fe, c["B"], c["B1"], np.ascontiguousarray(b[ok]))
            status[ok] = 1 | (inl.astype(np.uint8) << 1)
        status.setflags(write=False)
        _STATUS[key] = status
    return _STATUS[key]


# ---------------------------------------------------------------------------------------------- the launch-size estimate
def cand_cap(fe):
    """FeBookDev::cand_cap of a stream (book_alloc, mskf_capi_ctx.cpp)."""
    return fe.grid_row * fe.grid_col * max(fe.grid_max_feature_num, 1) + 8


def estimate(cand_caps, n_cand_last):
    """The max_pts of a frame batch's second track launch, restated from mskf_fe_frame_batch_begin (mskf_capi_fe.cpp): per
    stream cand_cap / 2 after mskf_fe_set_grid (n_cand_last < 0), else min(cand_cap, last + last / 2 + 32); the largest of the
    batch, at least 4."""
    est = 0
    for cap, last in zip(cand_caps, n_cand_last):
        est = max(est, cap // 2 if last < 0 else min(cap, last + last // 2 + 32))
    return max(est, 4)


# ---------------------------------------------------------------------------------------------- the frame sequence
FW, FH = 188, 120
SEED = 0x5EED0032
N_FRAMES = 8
FLAT = (3, 4)                                          # the drought: flat grey 128
_SEQ = {}


def frame_fe_cfg(compat=None):
    from msckf_stereo_c_amd.ctypes_types import COMPAT_REFERENCE, default_fe_cfg
    return default_fe_cfg(grid_row=6, grid_col=8, grid_min=3, grid_max=4, compat=COMPAT_REFERENCE if compat is None else compat)


def sequence(oracle):
    """(calib, [(cam0, cam1)] * 8): frames 0 .. 2 and 5 .. 7 rendered, 3 and 4 flat."""
    if not _SEQ:
        syn = oracle.Synth(seed=SEED, width=FW, height=FH)
        flat = np.full((FH, FW), 128, np.uint8)
        _SEQ["calib"] = syn.calib
        _SEQ["frames"] = [(flat, flat) if k in FLAT else tuple(np.ascontiguousarray(x) for x in syn.render(k)) for k in range(N_FRAMES)]
        for a, b in _SEQ["frames"]:
            a.setflags(write=False)
            b.setflags(write=False)
    return _SEQ["calib"], _SEQ["frames"]


def maxima_above_threshold(oracle, img, fe):
    """The detector's per-cell maxima that pass the threshold (score > fast_threshold * 256): what a frame's candidates are
    chosen from."""
    m = oracle.cell_maxima(img, fe.det_rows, fe.det_cols)
    return m[m["score"] > fe.fast_threshold * 256]


def track_reference(oracle, calib, fe, prev0, curr0, curr1, pts):
    """The oracle's answer for the first track launch of a frame on the previous grid's cam0 points `pts` (identity guess):
    oracle.lk_track, the bounds gate, oracle.stereo_match, oracle.undistort.  ok / inl are per input point; cam0, cam1, und0,
    und1 are per input point too (rows of points that are not ok are zero)."""
    pts = np.ascontiguousarray(pts, dtype=np.float32).reshape(-1, 2)
    n = len(pts)
    h, w = curr0.shape
    out = dict(ok=np.zeros(n, bool), inl=np.zeros(n, bool), **{k: np.zeros((n, 2), np.float32) for k in ("cam0", "cam1", "und0", "und1")})
    if n:
        b, st = oracle.lk_track(prev0, curr0, pts, pts)
        ok = st.astype(bool) & LC.in_image(b, w, h)
        out["ok"] = ok
        if ok.any():
            sub = stereo_reference(oracle, calib, fe, curr0, curr1, b[ok])
            out["inl"][ok] = sub["inl"]
            for k in ("cam0", "cam1", "und0", "und1"):
                out[k][ok] = sub[k]
    out["before_tracking"], out["after_tracking"], out["after_matching"] = n, int(out["ok"].sum()), int(out["inl"].sum())
    return out


def stereo_reference(oracle, calib, fe, curr0, curr1, pts0):
    """oracle.stereo_match and oracle.undistort of cam0 points of the current pair."""
    pts0 = np.ascontiguousarray(pts0, dtype=np.float32).reshape(-1, 2)
    K0, D0 = np.array(calib.cam0_intrinsics), np.array(calib.cam0_distortion)
    K1, D1 = np.array(calib.cam1_intrinsics), np.array(calib.cam1_distortion)
    c1, inl = oracle.stereo_match(calib, fe, curr0, curr1, pts0)
    return dict(cam0=pts0, cam1=c1, inl=inl.astype(bool), und0=oracle.undistort(K0, D0, pts0, model=calib.cam0_model),
                und1=oracle.undistort(K1, D1, c1, model=calib.cam1_model))
