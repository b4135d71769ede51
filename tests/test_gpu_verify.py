"""The opt-in geometric verification on the device (k_fe_verify; mskf_fe_verify*; Runner.verify_keyframes) against the Python
restatement of the contract (tests/verify_reference.py; DESIGN.md section 3, "Geometric verification"), bit for bit: the kernel
launched directly over every job of tests/verify_cases.py in one launch with the keys between guard words, the C ABI single, batched
and begin / end with other work of the context between, every refusal, and the Runner's keyframes on two synthetic streams."""
import ctypes as C

import numpy as np
import pytest

import brief_cases as BC
import match_cases as MC
import verify_cases as VC
import verify_reference as VR
from msckf_stereo_c_amd import capi
from msckf_stereo_c_amd.ctypes_types import FeVerifyArgs, default_ekf_cfg, default_fe_cfg

from hip_runtime import Hip
from test_verify_reference import BY_NAME, FeVerifyDev, _angle, _same, reference, staged

pytestmark = pytest.mark.gpu

GUARD = 0xEEEEEEEEEEEEEEEE
_HIP_ERRORS = []                              # after a HIP error no test of this module launches anything


# ------------------------------------------------------------------------------------------ the kernel, launched directly
def _blocks(K):
    return (K + VR.HYP_BLOCK - 1) // VR.HYP_BLOCK


def _launch(gpu_ctx, cases, max_K=None):
    """One fe_launch_verify over the cases' staged pairs.  Returns the merged key of every job; the guard words around every job's
    keys and the inputs are checked to be untouched."""
    assert not _HIP_ERRORS, "an earlier launch ended with a HIP error: %s" % _HIP_ERRORS
    f = gpu_ctx.L.fe_launch_verify
    f.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    f.restype = None
    hip = Hip()
    try:
        in_off, n_in = [], 8
        for c in cases:
            in_off.append(n_in)
            n_in += VR.PAIR * len(staged(c)[1]) + 8                        # 8 doubles of 0xA5 bytes between the jobs' pairs
        host_in = np.frombuffer(np.full(8 * n_in, 0xA5, np.uint8).tobytes(), np.float64).copy()
        for c, o in zip(cases, in_off):
            p = staged(c)[1]
            host_in[o:o + p.size] = p.reshape(-1)
        key_off, n_out = [], 1
        for c in cases:
            key_off.append(n_out)
            n_out += _blocks(c["n_hypotheses"]) + 1                         # one guard word between the jobs' keys
        host_out = np.full(n_out, GUARD, np.uint64)
        d_in, d_out = hip.alloc(8 * n_in, False), hip.alloc(8 * n_out, False)
        hip.put(d_in, host_in.view(np.uint8))
        hip.put(d_out, host_out.view(np.uint8))
        jobs = (FeVerifyDev * len(cases))()
        for j, c, o, ko in zip(jobs, cases, in_off, key_off):
            cam, pairs, _, e2max = staged(c)
            n, K = len(pairs), c["n_hypotheses"]
            assert 0 <= n <= VR.MAX_N and 1 <= K <= VR.MAX_K and o + VR.PAIR * n <= n_in and ko + _blocks(K) <= n_out          # what keeps every access inside
            j.pairs, j.keys = d_in + 8 * o, d_out + 8 * ko
            j.cam.R[:], j.cam.t[:] = cam[0], cam[1]
            j.seed, j.max_error2, j.min_depth, j.n, j.K = c["seed"], e2max, c["min_depth"], n, K
        raw = np.frombuffer(bytes(jobs), np.uint8).copy()
        d_jobs = hip.alloc(raw.size, False)
        hip.put(d_jobs, raw)
        f(d_jobs, len(cases), max(c["n_hypotheses"] for c in cases) if max_K is None else max_K, gpu_ctx.hip_stream())
        gpu_ctx.sync()
        err = hip.last_error()
        assert err == 0, "hipGetLastError %d after k_fe_verify" % err
        got = hip.get(d_out, 8 * n_out).view(np.uint64)
        assert np.array_equal(hip.get(d_in, 8 * n_in), host_in.view(np.uint8))
    except BaseException as e:
        _HIP_ERRORS.append(repr(e))
        raise
    finally:
        hip.free()
    inside = np.zeros(n_out, bool)
    keys = []
    for c, ko in zip(cases, key_off):
        b = _blocks(c["n_hypotheses"])
        inside[ko:ko + b] = True
        keys.append(max(int(v) for v in got[ko:ko + b]))                    # fv_merge
    assert np.all(got[~inside] == GUARD), "a word landed outside the key arrays"
    return keys, [got[ko:ko + _blocks(c["n_hypotheses"])].copy() for c, ko in zip(cases, key_off)]


_keys = {}


def want_key(c):
    """(merged key, the key of every block of 64 hypotheses) by the restatement, computed once."""
    if c["name"] not in _keys:
        cam, pairs, _, e2max = staged(c)
        key, counts = VR.score(cam, pairs, c["seed"], c["n_hypotheses"], c["min_depth"], e2max)
        per_h = [VR.KEY_NONE if m < 0 else VR.key_of(m, h) for h, m in enumerate(counts)]
        _keys[c["name"]] = (key, [max(per_h[b:b + VR.HYP_BLOCK]) for b in range(0, len(per_h), VR.HYP_BLOCK)])
    return _keys[c["name"]]


def test_direct_every_case_in_one_launch(gpu_ctx):
    """Every job of verify_cases.py (usable n = 3 .. 4096 at the wavefront and tile edges, K = 1 .. 1024 at the workgroup edges, the
    jobs with fewer than three pairs and with void triads only between the others) in ONE launch: every workgroup's key."""
    assert any(len(staged(c)[1]) == 0 for c in VC.CASES) and any(len(staged(c)[1]) == 4096 and c["n_hypotheses"] == 1024 for c in VC.CASES)
    keys, blocks = _launch(gpu_ctx, VC.CASES)
    for c, key, per_block in zip(VC.CASES, keys, blocks):
        want, want_blocks = want_key(c)
        assert per_block.tolist() == want_blocks, (c["name"], "block keys")
        assert key == want and VR.key_h(key) == reference(c)["best"], c["name"]


def test_direct_launch_cut_for_more_hypotheses_than_a_job_has(gpu_ctx):
    """A launch cut for 1024 hypotheses over jobs that have fewer: the workgroups beyond a job's K write nothing."""
    cases = [BY_NAME[n] for n in ("size 3x1", "n = 0", "size 64x65", "all points collinear", "noisy 48", "size 4x63")]
    keys, _ = _launch(gpu_ctx, cases, max_K=1024)
    assert keys == [want_key(c)[0] for c in cases]


# ------------------------------------------------------------------------------------------ through the C ABI
ABI_NAMES = ["size 3x1", "size 65x256", "n = 0", "n = 2", "three identical points", "all points collinear", "noise-free, no outliers",
             "points behind the keyframe camera", "usable mask and zero disparity", "noisy 48", "size %dx65" % (VR.TILE + 1)]


def _status(call, *a, **kw):
    try:
        call(*a, **kw)
        return 0
    except capi.MskfError as e:
        return e.code


def test_abi_single_calls(gpu_ctx):
    for name in ABI_NAMES:
        c = BY_NAME[name]
        _same(gpu_ctx.verify(**VC.options(c)), reference(c), name)


def test_abi_batch_of_every_case(gpu_ctx):
    """One batch of every job (unequal n and K, empty ones, the largest); twice, so that the second runs in the grown arenas.  A job
    alone (test_abi_single_calls) equals the same job inside this batch: both equal the restatement."""
    jobs = [VC.options(c) for c in VC.CASES]
    for rep in range(2):
        for c, got in zip(VC.CASES, gpu_ctx.verify_batch(jobs)):
            _same(got, reference(c), (c["name"], rep))
    alone = gpu_ctx.verify(**VC.options(BY_NAME["size 437x256"]))
    _same(alone, gpu_ctx.verify_batch(jobs[:9])[[c["name"] for c in VC.CASES].index("size 437x256")], "alone == in a batch")


def test_abi_begin_end_with_other_work_between(gpu_ctx, oracle):
    """Between _begin and _end the context pushes images, describes and matches; a second _begin while one is pending is refused and
    leaves the pending one alone; a batch without a pair leaves nothing pending."""
    w, h = 129, 71
    s = capi.Stream(gpu_ctx, oracle.euroc_calib(w, h), default_fe_cfg(), default_ekf_cfg())
    cases = [BY_NAME[n] for n in ABI_NAMES]
    gpu_ctx.verify_batch_begin([VC.options(c) for c in cases])
    s.push_stereo(BC.image("blocks", w, h, seed=20), BC.image("smooth", w, h, seed=21))
    desc, valid = gpu_ctx.describe_batch([s], [1], [BC.lattice(w, h)])[0]
    m, n_matches = gpu_ctx.match(desc, desc, valid, valid)
    assert n_matches > 0
    other = BY_NAME["noisy 48"]
    assert _status(gpu_ctx.verify, **VC.options(other)) == -1 and b"verify batch" in gpu_ctx.L.mskf_last_error()
    pending = gpu_ctx._vfy_pending
    assert _status(gpu_ctx.verify_batch_begin, [VC.options(other)]) == -1 and b"still pending" in gpu_ctx.L.mskf_last_error()
    assert gpu_ctx._vfy_pending is pending                # the refused wrapper call has not replaced the pending record's buffers
    for c, got in zip(cases, gpu_ctx.verify_batch_end()):
        _same(got, reference(c), c["name"])
    assert gpu_ctx.verify_batch_end() is None             # nothing pending: a no-op
    # a batch whose every n is 0 (and one without a hypothesis anywhere): outputs filled by _begin, nothing pending
    empty = [BY_NAME["n = 0"], BY_NAME["n = 0"], BY_NAME["n = 2"]]
    gpu_ctx.verify_batch_begin([VC.options(c) for c in empty])
    args = gpu_ctx._vfy_pending[1]
    assert [(args[i].status, args[i].best, args[i].n_usable) for i in range(3)] == [(1, -1, 0), (1, -1, 0), (1, -1, 2)]
    _same(gpu_ctx.verify(**VC.options(other)), reference(other), "after the empty batch: not refused")
    for c, got in zip(empty, gpu_ctx.verify_batch_end()):
        _same(got, reference(c), c["name"])
    s.close()


def test_abi_refusals(gpu_ctx):
    """Every refusal is MSKF_ERR_INVALID with a reason, leaves the outputs untouched and nothing pending."""
    L = gpu_ctx.L
    L.mskf_fe_verify.argtypes = [C.c_void_p, C.c_void_p]
    L.mskf_fe_verify_batch.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    L.mskf_fe_verify_batch_begin.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    L.mskf_fe_verify_batch_end.argtypes = [C.c_void_p]
    c = BY_NAME["noisy 48"]
    q, t = c["query_obs"], c["train_obs"]
    inl = np.full(len(q), 0xEE, np.uint8)

    def args(inlier=inl, **kw):
        a = FeVerifyArgs()
        a.n, a.n_hypotheses, a.query_obs, a.train_obs, a.usable = len(q), c["n_hypotheses"], q.ctypes.data, t.ctypes.data, None
        a.T_cam1_cam0[:] = c["T_cam1_cam0"].reshape(-1).tolist()
        a.seed, a.max_error, a.min_depth, a.max_depth, a.inlier = c["seed"], c["max_error"], c["min_depth"], c["max_depth"], inlier.ctypes.data
        a.n_usable = a.n_inliers = a.best = a.status = -9
        a.rms = -9.0
        for k, v in kw.items():
            if k == "T":
                a.T_cam1_cam0[v[0]] = v[1]
            else:
                setattr(a, k, v)
        return a

    def untouched(a):
        return (a.n_usable, a.n_inliers, a.best, a.status, a.rms) == (-9, -9, -9, -9, -9.0) and not any(a.R[:]) and not any(a.info[:])

    def refused(rc, text, a=None):
        assert rc == -1 and text in L.mskf_last_error(), (rc, L.mskf_last_error())
        assert (inl == 0xEE).all() and (a is None or untouched(a)), text
        _same(gpu_ctx.verify(**VC.options(c)), reference(c), text)         # nothing pending, the context usable

    good = args()
    refused(L.mskf_fe_verify(None, C.byref(good)), b"null argument", good)
    refused(L.mskf_fe_verify(gpu_ctx.h, None), b"null argument")
    refused(L.mskf_fe_verify_batch(gpu_ctx.h, 1, None), b"null argument")
    refused(L.mskf_fe_verify_batch(gpu_ctx.h, 0, C.byref(good)), b"at least one job", good)
    refused(L.mskf_fe_verify_batch(gpu_ctx.h, -1, C.byref(good)), b"at least one job", good)
    nan, inf = float("nan"), float("inf")
    for kw, text in [(dict(n=-1), b"negative"), (dict(n=4097), b"4096"), (dict(query_obs=None), b"null query_obs"), (dict(train_obs=None), b"null train_obs"),
                     (dict(n_hypotheses=0), b"n_hypotheses"), (dict(n_hypotheses=1025), b"n_hypotheses"), (dict(n_hypotheses=-3), b"n_hypotheses"),
                     (dict(max_error=0.0), b"max_error"), (dict(max_error=-1.0), b"max_error"), (dict(max_error=nan), b"max_error"), (dict(max_error=inf), b"max_error"),
                     (dict(min_depth=0.0), b"depths"), (dict(min_depth=-1.0), b"depths"), (dict(min_depth=nan), b"depths"), (dict(max_depth=nan), b"depths"),
                     (dict(max_depth=inf), b"depths"), (dict(min_depth=2.0, max_depth=2.0), b"depths"), (dict(min_depth=3.0, max_depth=2.0), b"depths"),
                     (dict(T=(3, nan)), b"T_cam1_cam0"), (dict(T=(5, inf)), b"T_cam1_cam0")]:
        a = args(**kw)
        refused(L.mskf_fe_verify(gpu_ctx.h, C.byref(a)), text, a)
        pair = (FeVerifyArgs * 2)(args(), args(**kw))                      # the second member of a batch: the first is not touched either
        refused(L.mskf_fe_verify_batch(gpu_ctx.h, 2, pair), text, pair[0])
        assert untouched(pair[1])
    # what is NOT refused: null pointers of an empty job, a null inlier array, one hypothesis, 4096 pairs (test_abi_batch_of_every_case)
    a = args(n=0, query_obs=None, train_obs=None, inlier=inl)
    a.inlier = None
    assert L.mskf_fe_verify(gpu_ctx.h, C.byref(a)) == 0 and (a.status, a.best, a.n_usable, a.n_inliers) == (1, -1, 0, 0)
    a = args(n_hypotheses=1)
    a.inlier = None
    assert L.mskf_fe_verify(gpu_ctx.h, C.byref(a)) == 0 and a.status in (0, 1, 2) and a.best in (-1, 0) and (inl == 0xEE).all()
    # a verify batch already pending
    pend = args()
    assert L.mskf_fe_verify_batch_begin(gpu_ctx.h, 1, C.byref(pend)) == 0
    inl2 = np.full(len(q), 0xEE, np.uint8)
    late = args(inlier=inl2)
    assert L.mskf_fe_verify(gpu_ctx.h, C.byref(late)) == -1 and b"still pending" in L.mskf_last_error()
    assert (inl2 == 0xEE).all() and untouched(late) and untouched(pend)
    assert L.mskf_fe_verify_batch_end(gpu_ctx.h) == 0
    want = reference(c)
    assert (pend.n_usable, pend.n_inliers, pend.best, pend.status) == tuple(want[k] for k in ("n_usable", "n_inliers", "best", "status"))
    assert np.array_equal(inl, want["inlier"]) and pend.R[:] == want["R"].reshape(-1).tolist() and pend.rms == want["rms"]


def test_a_context_that_never_verifies_allocates_nothing_for_it(oracle):
    """The arenas of the call are empty until the first call that launches (a job without a hypothesis does not)."""
    ctx = capi.Context(0)
    L = ctx.L
    L.fe_verify_arena_bytes.argtypes = [C.c_void_p]
    L.fe_verify_arena_bytes.restype = C.c_size_t
    w, h = 129, 71
    s = capi.Stream(ctx, oracle.euroc_calib(w, h), default_fe_cfg(), default_ekf_cfg())
    s.push_stereo(BC.image("blocks", w, h, seed=20), BC.image("smooth", w, h, seed=21))
    desc, valid = ctx.describe_batch([s], [1], [BC.lattice(w, h)])[0]
    ctx.match(desc, desc, valid, valid)
    assert L.fe_verify_arena_bytes(ctx.h) == 0
    _same(ctx.verify(**VC.options(BY_NAME["n = 2"])), reference(BY_NAME["n = 2"]), "no hypothesis")
    assert L.fe_verify_arena_bytes(ctx.h) == 0
    _same(ctx.verify(**VC.options(BY_NAME["noisy 48"])), reference(BY_NAME["noisy 48"]), "a job")
    assert L.fe_verify_arena_bytes(ctx.h) > 0
    s.close()
    ctx.close()


def test_every_kind_of_batch_on_one_context_then_verify(oracle):
    """A context claims a completion-mark slot per kind of pending batch at its first use (spinning waits, the default).  The
    verify batch is the ninth kind beside the detector's mark, the context's wait, track, frame, describe, match, update and
    read-out: one fresh context uses them all, and the verify call is not refused for want of a slot."""
    ctx = capi.Context(0)
    L = ctx.L
    L.mskf_ctx_set_wait_mode.argtypes = [C.c_void_p, C.c_int]
    assert L.mskf_ctx_set_wait_mode(ctx.h, 0) == 0          # spinning waits, whatever the environment says
    L.fe_mark_slots_used.argtypes = [C.c_void_p]
    w, h = 752, 480                                         # (a size at which whole frames run on the device)
    s = capi.Stream(ctx, oracle.euroc_calib(w, h), default_fe_cfg(), default_ekf_cfg())
    a, b = BC.image("blocks", w, h, seed=20), BC.image("smooth", w, h, seed=21)
    s.push_stereo(a, b)
    ctx.sync()
    cm = s.cell_maxima()
    pts = np.stack([cm["x"], cm["y"]], 1)[:20]
    ctx.track_batch([s], [dict(pts=pts, do_temporal=0)])
    assert s.grid_capacity() > 0
    s.swap()
    s.set_grid()
    ctx.frame_batch_begin([s], [(a, b)], [{}])
    ctx.frame_batch_end()
    desc, valid = ctx.describe_batch([s], [1], [BC.lattice(w, h)])[0]
    ctx.match(desc, desc, valid, valid)
    H = np.zeros((1, 21))
    H[0, 12] = 1.0
    s.ekf_update_direct(H, [0.01], [[0.25]])
    s.ekf_pos_var()
    ctx.sync()
    before = L.fe_mark_slots_used(ctx.h)
    c = BY_NAME["noisy 48"]
    _same(ctx.verify(**VC.options(c)), reference(c), "the ninth kind")
    assert (before, L.fe_mark_slots_used(ctx.h)) == (8, 9)
    s.close()
    ctx.close()


def test_wait_mode_is_refused_while_any_kind_is_pending(oracle):
    """A completion mark recorded in one wait mode cannot be awaited in the other, so mskf_ctx_set_wait_mode refuses between the
    _begin and the _end of every kind of batch: each of the seven in turn, with the smallest job that launches, on the context and
    stream of the test above."""
    ctx = capi.Context(0)
    L = ctx.L
    L.mskf_ctx_set_wait_mode.argtypes = [C.c_void_p, C.c_int]
    assert L.mskf_ctx_set_wait_mode(ctx.h, 0) == 0
    w, h = 752, 480                                         # (a size at which whole frames run on the device)
    s = capi.Stream(ctx, oracle.euroc_calib(w, h), default_fe_cfg(), default_ekf_cfg())
    a, b = BC.image("blocks", w, h, seed=20), BC.image("smooth", w, h, seed=21)
    s.push_stereo(a, b)
    ctx.sync()
    cm = s.cell_maxima()
    pts = np.stack([cm["x"], cm["y"]], 1)[:20].astype(np.float32)
    assert len(pts) == 20 and s.grid_capacity() > 0

    def pending(kind, begin, end):
        begin()
        assert L.mskf_ctx_set_wait_mode(ctx.h, 1) == -1 and b"pending" in L.mskf_last_error(), kind
        end()
        assert L.mskf_ctx_set_wait_mode(ctx.h, 0) == 0, kind

    pending("track", lambda: ctx.track_batch_begin([s], [dict(pts=pts, do_temporal=0)]), ctx.track_batch_end)
    s.swap()
    und = (pts - np.float32([w / 2, h / 2])) / np.float32(VC.FX)
    s.set_grid(id=np.arange(20), lifetime=np.ones(20), cam0=pts, cam1=pts, und0=und, und1=und, next_feature_id=20)
    pending("device frame", lambda: ctx.frame_batch_begin([s], [(a, b)], [{}]), ctx.frame_batch_end)
    s.push_stereo(a, b)
    pending("describe", lambda: ctx.describe_batch_begin([s], [1], [pts]), ctx.describe_batch_end)
    mc = next(c for c in MC.CASES if c["name"] == "size 1x1")
    pending("match", lambda: ctx.match_batch_begin([MC.options(mc)]), ctx.match_batch_end)
    pending("verify", lambda: ctx.verify_batch_begin([VC.options(BY_NAME["size 3x1"])]), ctx.verify_batch_end)
    H = np.zeros((1, 21))
    H[0, 12] = 1.0
    pending("direct update", lambda: ctx.ekf_update_direct_batch_begin([s], [dict(H=H, r=[0.01], R=[[0.25]])]), ctx.ekf_update_direct_batch_end)
    pending("position-variance read-out", lambda: ctx.ekf_pos_var_batch_begin([s]), ctx.ekf_pos_var_batch_end)
    s.close()
    ctx.close()


# ------------------------------------------------------------------------------------------ the Runner's keyframes
def _hamilton(q):
    x, y, z, w = (float(v) for v in q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def _gt_motion(syn, kq, kk):
    """(R, t) of p_keyframe = R p_query + t in cam0 coordinates between frames kq and kk, from the generator's ground truth."""
    Tci = np.array(syn.calib.T_cam0_imu).reshape(4, 4)
    Rci, tci = Tci[:3, :3], Tci[:3, 3]
    Rwc, c = [], []
    for k in (kq, kk):
        g = syn.gt_pose(k)
        R_wi, p = _hamilton(g["q"]), np.array(g["p"], np.float64)
        Rwc.append(Rci @ R_wi.T)
        c.append(p - R_wi @ Rci.T @ tci)
    return Rwc[1] @ Rwc[0].T, Rwc[1] @ (c[0] - c[1])


def _frame_obs(run, stream):
    """(ids, float64[n, 4]) of the stream's last frame: what msg publishes for the described features."""
    ids = run.descriptors(stream)[0]
    m = run.msg(stream)[:len(ids)]
    assert np.array_equal(m["id"], ids.astype(m["id"].dtype))
    return ids, np.stack([m["u0"], m["v0"], m["u1"], m["v1"]], axis=1).astype(np.float64)


def _restated(run, stream, hit, fx, **kw):
    """VR.verify on what keyframe_obs, msg and query_keyframes return for one hit, and the hit's pairs."""
    k, _, n_matches, pairs = hit
    ids, obs = _frame_obs(run, stream)
    kf_ids, kf_obs = run.keyframe(stream, k)[1], run.keyframe_obs(stream, k)
    qi = [int(np.flatnonzero(ids == a)[0]) for a in pairs[:, 0]]
    ti = [int(np.flatnonzero(kf_ids == b)[0]) for b in pairs[:, 1]]
    opts = dict(dict(n_hypotheses=256, seed=0, min_depth=0.1, max_depth=40.0, max_error=2.0 / fx), **kw)
    return VR.verify(obs[qi].reshape(-1, 4), kf_obs[ti].reshape(-1, 4), np.array(run.calib.T_cam1_cam0).reshape(4, 4), **opts)


def _same_as_restated(got, want, pairs, what):
    k, t, n_matches, n_inliers, R, tr, info, rms, inlier_pairs = got
    assert (n_matches, n_inliers, want["status"]) == (len(pairs), want["n_inliers"], 0), what
    for a, b in ((R, want["R"]), (tr, want["t"]), (info, want["info"]), (np.float64(rms), np.float64(want["rms"]))):
        assert np.ascontiguousarray(a, np.float64).tobytes() == np.ascontiguousarray(b, np.float64).tobytes(), (what, a, b)
    assert np.array_equal(inlier_pairs, pairs[want["inlier"] != 0]), what


# Measured (the restatement on what the device tracked, which the device's result equals bit for bit; frame 14 against the keyframe
# of frame 6, stream 0, 188 x 120 images): 60 pairs, all usable, 59 inliers; the ground-truth motion is 1.263e-2 rad and 8.992e-2 m,
# the verified motion is 3.179e-3 rad and 2.338e-2 m from it.  (At the keyframe's own frame: 63 pairs, 63 inliers, 8.814e-4 rad and
# 6.183e-3 m from the identity: a few features of these small images share a descriptor with a neighbour and pair with it.)
# The asserted bars are three times these.
LATER_ROT_ERR_RAD = 3.179e-3
LATER_TRANS_ERR_M = 2.338e-2


def test_runner_verify_keyframes(oracle):
    from msckf_stereo_c_amd import runner as R
    w, h, n_frames, kf_at, kf_other, later = 188, 120, 15, 6, 9, 14
    syns = [oracle.Synth(seed=0x5EED00E0 + i, width=w, height=h, n_static=3) for i in range(2)]
    run = R.Runner(syns[0].calib, default_fe_cfg(), default_ekf_cfg(max_cam_state_size=10), 1, 2)
    run.set_descriptors(True)
    fx = float(syns[0].calib.cam0_intrinsics[0])
    assert run.verify_keyframes(0) == []                   # no query yet: nothing to verify
    j = 0
    for k in range(n_frames):
        t_img = syns[0].frame_time(k)
        while True:
            smp = [syn.imu(j) for syn in syns]
            j += 1
            for i, s in enumerate(smp):
                run.imu(i, s)
            if not (smp[0].time_stamp <= t_img):
                break
        frames = [syn.render(k) for syn in syns]
        run.step([f[0] for f in frames], [f[1] for f in frames], [t_img] * 2)
        if k == kf_at:
            assert run.add_keyframe(0) == 0
            ids, obs = _frame_obs(run, 0)
            assert np.array_equal(run.keyframe(0, 0)[1], ids) and np.array_equal(run.keyframe_obs(0, 0), obs) and len(ids) >= 5
            # at the keyframe's own frame: the motion is the identity, and every usable self-match is an inlier
            hits = run.query_keyframes(0)
            assert [hk for hk, _, _, _ in hits] == [0]
            got = run.verify_keyframes(0, min_inliers=0)
            want = _restated(run, 0, hits[0], fx)
            print("self-match: %d pairs, %d usable, %d inliers, rotation %.3e rad, translation %.3e m" % (
                len(hits[0][3]), want["n_usable"], want["n_inliers"], _angle(want["R"], np.eye(3)), np.linalg.norm(want["t"])))
            assert want["status"] == 0 and want["n_usable"] >= 3 and want["n_inliers"] == want["n_usable"]
            assert len(got) == 1
            _same_as_restated(got[0], want, hits[0][3], "self")
            assert _angle(got[0][4], np.eye(3)) <= 3 * _angle(want["R"], np.eye(3)) and np.linalg.norm(got[0][5]) <= 3 * np.linalg.norm(want["t"])
            # min_inliers is the runner's filter
            assert run.verify_keyframes(0, min_inliers=want["n_inliers"] + 1) == [] and len(run.verify_keyframes(0, min_inliers=want["n_inliers"])) == 1
        if k == kf_other:
            assert run.add_keyframe(1) == 0               # a second stream's keyframe: stream 0 does not see it
    # at a later frame: equal to the restatement on what keyframe_obs, msg and query_keyframes return, bit for bit
    hits = run.query_keyframes(0)
    assert [hk for hk, _, _, _ in hits] == [0] and run.num_keyframes(0) == 1
    for kw in (dict(), dict(n_hypotheses=64, seed=5, max_error=4.0 / fx), dict(n_hypotheses=1000, max_depth=25.0)):
        got = run.verify_keyframes(0, min_inliers=0, **kw)
        want = _restated(run, 0, hits[0], fx, **kw)
        if want["status"] != 0:
            assert got == [], kw
            continue
        assert len(got) == 1 and got[0][0] == 0 and got[0][1] == syns[0].frame_time(kf_at)
        _same_as_restated(got[0], want, hits[0][3], kw)
    # its motion agrees with the ground truth
    got = run.verify_keyframes(0, min_inliers=0)
    want = _restated(run, 0, hits[0], fx)
    Rg, tg = _gt_motion(syns[0], later, kf_at)
    rot_err, trans_err = _angle(want["R"], Rg), float(np.linalg.norm(want["t"] - tg))
    print("later frame: %d pairs, %d usable, %d inliers, status %d; ground-truth motion %.3e rad, %.3e m; rotation error %.3e rad, translation error %.3e m" % (
        len(hits[0][3]), want["n_usable"], want["n_inliers"], want["status"], _angle(Rg, np.eye(3)), np.linalg.norm(tg), rot_err, trans_err))
    assert np.linalg.norm(tg) > 0.02                       # the rig has moved
    assert want["status"] == 0 and len(got) == 1
    assert _angle(got[0][4], Rg) <= 3 * LATER_ROT_ERR_RAD and np.linalg.norm(got[0][5] - tg) <= 3 * LATER_TRANS_ERR_M
    # keyframes of another stream are not seen: stream 1 verifies against its own keyframe only
    assert [hk for hk, _, _, _ in run.query_keyframes(1)] == [0]
    v1 = run.verify_keyframes(1, min_inliers=0)
    assert len(v1) <= 1 and all(v[0] == 0 and v[1] == syns[1].frame_time(kf_other) for v in v1)
    # bad thresholds are the ABI's refusal
    with pytest.raises(R.MskfError, match="max_error"):
        run.verify_keyframes(0, max_error=-1.0)
    with pytest.raises(R.MskfError, match="n_hypotheses"):
        run.verify_keyframes(0, n_hypotheses=2000)
    # stale hits are refused: a newer frame has been described since the query
    k = n_frames
    t_img = syns[0].frame_time(k)
    while True:
        smp = [syn.imu(j) for syn in syns]
        j += 1
        for i, s in enumerate(smp):
            run.imu(i, s)
        if not (smp[0].time_stamp <= t_img):
            break
    frames = [syn.render(k) for syn in syns]
    run.step([f[0] for f in frames], [f[1] for f in frames], [t_img] * 2)
    with pytest.raises(R.MskfError, match="another frame"):
        run.verify_keyframes(0)
    run.query_keyframes(0)
    run.verify_keyframes(0)                                # after a new query: accepted again
    # descriptors switched off and on with no frame between: the frame's lists are gone, the time is unchanged; refused, not a crash
    assert len(run.query_keyframes(0)) == 1
    run.set_descriptors(False, stream=0)
    run.set_descriptors(True, stream=0)
    with pytest.raises(R.MskfError, match="no longer among"):
        run.verify_keyframes(0)
    run.close()


def test_published_pose_has_the_convention_the_position_helper_assumes(oracle):
    """imu_position_from_verification reads a POSE record's q as the rotation IMU -> world.  The turn between two poses that
    Runner.poses publishes, read that way, is the ground truth's turn between the same frames (both are turns in the IMU's own
    frame, so the filter's free yaw does not enter); read the other way round it is not.  The bar is a quarter of the angle
    turned: a filter that has lost its attitude by that much in a second would fail every other test first, and the wrong
    reading is off by about the angle itself."""
    from msckf_stereo_c_amd import runner as R
    syn = oracle.Synth(seed=0x5EED0000, width=376, height=240)
    run = R.Runner(syn.calib, default_fe_cfg(), default_ekf_cfg(), 1, 1)
    j = 0
    for k in range(60):
        t_img = syn.frame_time(k)
        while True:
            s = syn.imu(j)
            j += 1
            run.imu(0, s)
            if not (s.time_stamp <= t_img):
                break
        a, b = syn.render(k)
        run.step([a], [b], [t_img])
    poses = run.poses(0)
    run.close()
    ka, kb = 32, 59
    pa = poses[np.argmin(np.abs(poses["t"] - syn.frame_time(ka)))]
    pb = poses[np.argmin(np.abs(poses["t"] - syn.frame_time(kb)))]
    assert abs(pa["t"] - syn.frame_time(ka)) < 1e-6 and abs(pb["t"] - syn.frame_time(kb)) < 1e-6
    Ga, Gb = R.pose_rotation(syn.gt_pose(ka)["q"]), R.pose_rotation(syn.gt_pose(kb)["q"])
    Pa, Pb = R.pose_rotation(pa["q"]), R.pose_rotation(pb["q"])
    turned, right, wrong = _angle(Ga, Gb), _angle(Pa.T @ Pb, Ga.T @ Gb), _angle(Pa @ Pb.T, Ga.T @ Gb)
    print("published poses: turned %.3e rad; as IMU -> world %.3e rad off the ground truth's turn, as world -> IMU %.3e rad" % (turned, right, wrong))
    assert turned > 0.05 and right < 0.25 * turned and wrong > 0.5 * turned
