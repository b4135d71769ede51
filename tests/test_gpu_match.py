"""The opt-in descriptor matcher on the device (k_fe_match; mskf_fe_match*; Runner keyframes) against the numpy restatement of the
contract (tests/match_reference.py; DESIGN.md section 3, "Descriptor matching"), bit for bit: the kernel launched directly over
every job of tests/match_cases.py in one launch with the outputs between guard bytes, the C ABI single, batched and begin / end with
other work of the context between, every refusal, describe -> match on real images, and the Runner's keyframes."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import brief_cases as BC
import lk_cases as LK
import match_cases as MC
import match_reference as MR
from msckf_stereo_c_amd import capi
from msckf_stereo_c_amd.ctypes_types import MATCH, FeMatchArgs, default_ekf_cfg, default_fe_cfg

from hip_runtime import Hip
from test_match_reference import BY_NAME, FIELDS, _same, reference

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 0xEE
_HIP_ERRORS = []                              # after a HIP error no test of this module launches anything


class FeMatchDev(C.Structure):
    """FeMatchDev of csrc/hip/fe_match.h: one job of a launch."""
    _fields_ = [("query", C.c_void_p), ("query_valid", C.c_void_p), ("train", C.c_void_p), ("train_valid", C.c_void_p), ("nq", C.c_int), ("nt", C.c_int),
                ("max_distance", C.c_int), ("ratio", C.c_float), ("cross_check", C.c_int), ("pad_", C.c_int), ("matches", C.c_void_p)]


def test_layouts_match_the_header(tmp_path):
    so = str(tmp_path / "libfe_match_test.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-I", ROOT, "-o", so, os.path.join(ROOT, "tests", "cpp", "fe_match_test.cpp")])
    out = (C.c_int * 32)()
    n = C.CDLL(so).fm_match_dev_layout(out, 32)
    dev = [C.sizeof(FeMatchDev)] + [getattr(FeMatchDev, k).offset for k in ("query", "query_valid", "train", "train_valid", "nq", "nt", "max_distance", "ratio",
                                                                            "cross_check", "matches")]
    assert list(out[:n]) == dev + [MATCH.itemsize] + [MATCH.fields[k][1] for k in FIELDS]
    assert MATCH == MR.MATCH


# ------------------------------------------------------------------------------------------ the kernel, launched directly
def _launch(gpu_ctx, cases, max_nq=None):
    """One fe_launch_match over the cases.  Returns [(matches, n_matches)]; the guard bytes around every output array and the
    inputs are checked to be untouched.  Descriptor sets lie at 16-byte aligned addresses (FeMatchDev asks for it), validity
    arrays and outputs at odd ones."""
    assert not _HIP_ERRORS, "an earlier launch ended with a HIP error: %s" % _HIP_ERRORS
    f = gpu_ctx.L.fe_launch_match
    f.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    f.restype = None
    hip = Hip()
    try:
        n_in, offs = 64, []
        for c in cases:
            o = {}
            for key, odd in (("query", 0), ("train", 0), ("query_valid", 1), ("train_valid", 1)):
                a = c[key]
                if a is None:
                    o[key] = None
                    continue
                o[key] = n_in + odd
                n_in += (a.size + odd + 63 + 64) // 64 * 64                # at least 63 bytes of 0xA5 behind every array
            offs.append(o)
        host_in = np.full(n_in, 0xA5, np.uint8)
        for c, o in zip(cases, offs):
            for key, at in o.items():
                if at is not None:
                    host_in[at:at + c[key].size] = c[key].reshape(-1)
        n_out, out_off = 13, []
        for c in cases:
            out_off.append(n_out)
            n_out += 12 * len(c["query"]) + 13                             # 13-byte guards: nothing is aligned
        host_out = np.full(n_out, GUARD, np.uint8)
        d_in, d_out = hip.alloc(n_in, False), hip.alloc(n_out, False)
        hip.put(d_in, host_in)
        hip.put(d_out, host_out)
        jobs = (FeMatchDev * len(cases))()
        for j, c, o, oo in zip(jobs, cases, offs, out_off):
            nq, nt = len(c["query"]), len(c["train"])
            assert nq <= MR.MAX_N and nt <= MR.MAX_N and (d_in + o["query"]) % 16 == 0 and (d_in + o["train"]) % 16 == 0       # what keeps every access inside
            j.query, j.train = d_in + o["query"], d_in + o["train"]
            j.query_valid = None if o["query_valid"] is None else d_in + o["query_valid"]
            j.train_valid = None if o["train_valid"] is None else d_in + o["train_valid"]
            j.nq, j.nt, j.max_distance, j.ratio, j.cross_check, j.matches = nq, nt, c["max_distance"], c["ratio"], int(c["cross_check"]), d_out + oo
        raw = np.frombuffer(bytes(jobs), np.uint8).copy()
        d_jobs = hip.alloc(raw.size, False)
        hip.put(d_jobs, raw)
        f(d_jobs, len(cases), max((len(c["query"]) for c in cases), default=0) if max_nq is None else max_nq, max((len(c["train"]) for c in cases), default=0),
          gpu_ctx.hip_stream())
        gpu_ctx.sync()
        err = hip.last_error()
        assert err == 0, "hipGetLastError %d after k_fe_match" % err
        got = hip.get(d_out, n_out)
        assert np.array_equal(hip.get(d_in, n_in), host_in)
    except BaseException as e:
        _HIP_ERRORS.append(repr(e))
        raise
    finally:
        hip.free()
    inside = np.zeros(n_out, bool)
    res = []
    for c, oo in zip(cases, out_off):
        nq = len(c["query"])
        inside[oo:oo + 12 * nq] = True
        m = got[oo:oo + 12 * nq].copy().view(MATCH)
        res.append((m, int((m["idx"] >= 0).sum())))
    assert np.all(got[~inside] == GUARD), "a byte landed outside the output arrays"
    return res


def test_direct_every_case_in_one_launch(gpu_ctx):
    """Every job of match_cases.py, the empty ones and the two with 65535 descriptors between the others, in ONE launch."""
    assert any(len(c["query"]) == 0 for c in MC.CASES) and any(len(c["train"]) == 0 and len(c["query"]) for c in MC.CASES)
    for c, got in zip(MC.CASES, _launch(gpu_ctx, MC.CASES)):
        _same(got, reference(c), c["name"])


def test_direct_a_workgroup_takes_several_query_blocks(gpu_ctx):
    """A launch cut for fewer queries than its largest job has."""
    cases = [BY_NAME[n] for n in ("size 129x%d" % (MR.TILE + 1), "size 0x64", "size 65x2", "edges invalid on both sides", "size 129x0", "size 64x%d" % (2 * MR.TILE + 1))]
    for c, got in zip(cases, _launch(gpu_ctx, cases, max_nq=40)):
        _same(got, reference(c), c["name"])


def test_direct_nothing_to_do(gpu_ctx):
    """No query anywhere: no launch, nothing written."""
    cases = [BY_NAME["size 0x64"], BY_NAME["size 0x0"]]
    assert [len(m) for m, _ in _launch(gpu_ctx, cases)] == [0, 0]


# ------------------------------------------------------------------------------------------ through the C ABI
ABI_NAMES = ["duplicate train", "all equal, cross-checked", "exactly one valid train", "ratio 0.8f, 4 against 5", "cross-check tie", "size 1x0", "size 0x2",
             "size 65x%d" % (MR.TILE + 1), "size 129x%d" % (2 * MR.TILE + 1), "size 63x63", "edges invalid on both sides", "all train invalid"]


def _status(call, *a, **kw):
    try:
        call(*a, **kw)
        return 0
    except capi.MskfError as e:
        return e.code


def test_abi_single_calls(gpu_ctx):
    for name in ABI_NAMES:
        c = BY_NAME[name]
        _same(gpu_ctx.match(**MC.options(c)), reference(c), name)


def test_abi_batch_of_every_case(gpu_ctx):
    """One batch of every job (unequal sizes, empty ones, both large ones); twice, so that the second runs in the grown arenas."""
    jobs = [MC.options(c) for c in MC.CASES]
    for rep in range(2):
        for c, got in zip(MC.CASES, gpu_ctx.match_batch(jobs)):
            _same(got, reference(c), (c["name"], rep))


def test_abi_eight_jobs_share_one_query(gpu_ctx):
    """A query against 8 keyframes: 8 jobs with one query pointer (and one validity pointer), copied once."""
    rng = np.random.default_rng(8)
    q = MC.rand_desc(rng, 130)
    qv = MC.edge_validity(130, 5)
    trains = [MC.near_set(rng, q, n) for n in (1, 70, 0, 257, 64, 300, 2, 129)]
    jobs = [dict(query=q, query_valid=qv, train=t, cross_check=k % 2 == 0, ratio=0.8, max_distance=10) for k, t in enumerate(trains)]
    got = gpu_ctx.match_batch(jobs)
    built = gpu_ctx.match_batch_begin(jobs)
    assert len(built) == 8
    args = gpu_ctx._mch_pending[1]
    assert len({args[i].query for i in range(8)}) == 1 and len({args[i].query_valid for i in range(8)}) == 1      # the ABI sees one pointer
    again = gpu_ctx.match_batch_end()
    for k, j in enumerate(jobs):
        want = MR.match(**j)
        _same(got[k], want, k)
        _same(again[k], want, k)


def test_abi_begin_end_with_other_work_between(gpu_ctx, oracle):
    """Between _begin and _end the context pushes images and runs a describe batch; a second _begin while one is pending is refused
    and leaves the pending one alone; an all-empty batch leaves nothing pending."""
    w, h = 129, 71
    s = capi.Stream(gpu_ctx, oracle.euroc_calib(w, h), default_fe_cfg(), default_ekf_cfg())
    cases = [BY_NAME[n] for n in ABI_NAMES]
    gpu_ctx.match_batch_begin([MC.options(c) for c in cases])
    a, b = BC.image("blocks", w, h, seed=20), BC.image("smooth", w, h, seed=21)
    s.push_stereo(a, b)
    pts = BC.lattice(w, h)
    desc = gpu_ctx.describe_batch([s], [1], [pts])[0]
    other = BY_NAME["size 1x2"]
    assert _status(gpu_ctx.match, **MC.options(other)) == -1 and b"match batch" in gpu_ctx.L.mskf_last_error()
    assert _status(gpu_ctx.match_batch_begin, [MC.options(other)]) == -1 and b"still pending" in gpu_ctx.L.mskf_last_error()
    # (the refused wrapper call has not replaced the pending record's buffers: the refusal comes before the wrapper stores anything)
    for c, got in zip(cases, gpu_ctx.match_batch_end()):
        _same(got, reference(c), c["name"])
    assert desc[1].any()
    assert gpu_ctx.match_batch_end() is None              # nothing pending: a no-op
    # a batch whose every nq is 0
    empty = [BY_NAME["size 0x64"], BY_NAME["size 0x0"]]
    gpu_ctx.match_batch_begin([MC.options(c) for c in empty])
    args = gpu_ctx._mch_pending[1]
    assert [args[i].n_matches for i in range(2)] == [0, 0]
    _same(gpu_ctx.match(**MC.options(other)), reference(other), "after the empty batch: not refused")
    assert [n for _, n in gpu_ctx.match_batch_end()] == [0, 0]
    s.close()


def test_abi_refusals(gpu_ctx):
    """Every refusal is MSKF_ERR_INVALID with a reason, leaves matches and n_matches untouched and nothing pending."""
    L = gpu_ctx.L
    L.mskf_fe_match.argtypes = [C.c_void_p, C.c_void_p]
    L.mskf_fe_match_batch.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    L.mskf_fe_match_batch_begin.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    c = BY_NAME["size 65x64"]
    q, t = c["query"], c["train"]
    out = np.full(12 * len(q), GUARD, np.uint8)

    def args(**kw):
        v = dict(nq=len(q), nt=len(t), query=q.ctypes.data, query_valid=None, train=t.ctypes.data, train_valid=None, max_distance=256, ratio=0.0,
                 cross_check=0, matches=out.ctypes.data, n_matches=-9)
        v.update(kw)
        return FeMatchArgs(**v)

    def refused(rc, text, a=None):
        assert rc == -1 and text in L.mskf_last_error(), (rc, L.mskf_last_error())
        assert (out == GUARD).all() and (a is None or a.n_matches == -9), text
        _same(gpu_ctx.match(**MC.options(c)), reference(c), text)          # nothing pending, the context usable

    good = args()
    refused(L.mskf_fe_match(None, C.byref(good)), b"null argument", good)
    refused(L.mskf_fe_match(gpu_ctx.h, None), b"null argument")
    refused(L.mskf_fe_match_batch(gpu_ctx.h, 1, None), b"null argument")
    refused(L.mskf_fe_match_batch(gpu_ctx.h, 0, C.byref(good)), b"at least one job", good)
    refused(L.mskf_fe_match_batch(gpu_ctx.h, -1, C.byref(good)), b"at least one job", good)
    for kw, text in [(dict(nq=-1), b"negative"), (dict(nt=-1), b"negative"), (dict(nq=65536), b"65535"), (dict(nt=65536), b"65535"),
                     (dict(query=None), b"null query"), (dict(train=None), b"null train"), (dict(matches=None), b"null matches"),
                     (dict(max_distance=-1), b"max_distance"), (dict(max_distance=257), b"max_distance"),
                     (dict(ratio=float("nan")), b"ratio"), (dict(ratio=-0.25), b"ratio"), (dict(ratio=1.0000001), b"ratio")]:
        a = args(**kw)
        refused(L.mskf_fe_match(gpu_ctx.h, C.byref(a)), text, a)
        pair = (FeMatchArgs * 2)(args(), args(**kw))                       # the second member of a batch: the first is not touched either
        refused(L.mskf_fe_match_batch(gpu_ctx.h, 2, pair), text, pair[0])
        assert pair[1].n_matches == -9
    # what is NOT refused: null pointers of empty sets, ratio 1.0, max_distance 0 and 256
    a = args(nq=0, query=None, matches=None)
    assert L.mskf_fe_match(gpu_ctx.h, C.byref(a)) == 0 and a.n_matches == 0
    a = args(nt=0, train=None, ratio=1.0, max_distance=0)
    assert L.mskf_fe_match(gpu_ctx.h, C.byref(a)) == 0 and a.n_matches == 0
    m = out.view(MATCH)
    assert (m["nearest"] == -1).all() and (m["dist"] == MR.NONE).all()
    out[:] = GUARD
    # a match batch already pending
    pend = args()
    assert L.mskf_fe_match_batch_begin(gpu_ctx.h, 1, C.byref(pend)) == 0
    out2 = np.full(12 * len(q), GUARD, np.uint8)
    late = args(matches=out2.ctypes.data)
    assert L.mskf_fe_match(gpu_ctx.h, C.byref(late)) == -1 and b"still pending" in L.mskf_last_error()
    assert (out2 == GUARD).all() and late.n_matches == -9
    L.mskf_fe_match_batch_end.argtypes = [C.c_void_p]
    assert L.mskf_fe_match_batch_end(gpu_ctx.h) == 0
    want = MR.match(q, t)
    _same((out.view(MATCH), pend.n_matches), want, "the pending batch itself")


# ------------------------------------------------------------------------------------------ describe -> match
def test_describe_then_match_on_real_images(gpu_ctx, oracle):
    """A stream pushed with the two views of one canvas (160 x 120, the second moved by (3, -2) with noise), the lattice described
    on both roles and matched: equal to numpy on the same arrays, and most points find themselves."""
    w, h, seed = 160, 120, 7
    canvas = LK.block_canvas(w, h, 8, seed)
    A = np.ascontiguousarray(LK.crop(canvas, w, h))
    noise = np.random.default_rng(seed).integers(-4, 5, (h, w))
    B = np.ascontiguousarray((LK.crop(canvas, w, h, 3, -2).astype(np.int64) + noise).clip(0, 255).astype(np.uint8))
    pts = np.array([(x, y) for y in range(20, h - 20, 9) for x in range(20, w - 20, 9)] + [(-3, 5), (w + 1, 7)], np.float32)
    s = capi.Stream(gpu_ctx, oracle.euroc_calib(w, h), default_fe_cfg(), default_ekf_cfg())
    s.push_stereo(A, B)
    (dA, vA), (dB, vB) = gpu_ctx.describe_batch([s, s], [1, 2], [pts, pts + np.array([3, -2], np.float32)])
    assert vA[:-2].all() and not vA[-2:].any()
    for kw in (dict(cross_check=True), dict(cross_check=True, ratio=0.8), dict(max_distance=40)):
        got = gpu_ctx.match(dA, dB, vA, vB, **kw)
        _same(got, MR.match(dA, dB, vA, vB, **kw), kw)
        if kw.get("cross_check"):
            assert (got[0]["idx"][:-2] == np.arange(len(pts) - 2)).sum() >= 100 and (got[0]["nearest"][-2:] == -1).all()
    s.close()


# ------------------------------------------------------------------------------------------ the Runner's keyframes
def _pairs_numpy(ids, desc, valid, kf, **kw):
    m, n = MR.match(desc, kf[2], valid, kf[3], **kw)
    hit = m["idx"] >= 0
    return n, np.stack([ids[hit], kf[1][m["idx"][hit]]], axis=1).astype(np.uint64).reshape(-1, 2)


def test_runner_keyframes(oracle):
    from msckf_stereo_c_amd import runner as R
    w, h, n_frames = 188, 120, 12
    syns = [oracle.Synth(seed=0x5EED00D0 + i, width=w, height=h) for i in range(2)]
    run = R.Runner(syns[0].calib, default_fe_cfg(), default_ekf_cfg(max_cam_state_size=10), 1, 2)
    run.set_descriptors(True)
    assert run.num_keyframes(0) == 0 and run.query_keyframes(0) == []
    kept, j = {}, 0
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
        ids, desc, valid = run.descriptors(0)
        if k in (3, 7):
            idx = run.add_keyframe(0)
            assert idx == len(kept) and run.num_keyframes(0) == idx + 1
            kf = run.keyframe(0, idx)
            assert kf[0] == t_img and np.array_equal(kf[1], ids) and np.array_equal(kf[2], desc) and np.array_equal(kf[3], valid) and len(ids) >= 5
            kept[idx] = kf
            # at the very frame of a keyframe: that keyframe comes back with the pairs numpy gives, every valid feature whose
            # descriptor no other feature of the frame shares against itself at distance 0
            hits = run.query_keyframes(0)
            assert [hk for hk, _, _, _ in hits] == list(range(idx + 1))
            hk, ht, hn, pairs = hits[-1]
            n, want = _pairs_numpy(ids, desc, valid, kf, cross_check=True)
            assert (hk, ht, hn) == (idx, t_img, n) and np.array_equal(pairs, want)
            d = MR.distances(desc, desc)
            alone = (valid != 0) & ((d == 0).sum(axis=1) == 1)
            assert alone.sum() >= 5 and {(int(i), int(i)) for i in ids[alone]} <= {tuple(int(v) for v in p) for p in pairs}
        if k == 5:
            assert run.add_keyframe(1) == 0          # a second stream's keyframe: stream 0 does not see it
    assert run.num_keyframes(0) == 2 and run.num_keyframes(1) == 1
    # at a later frame: equal to numpy on what descriptors() and keyframe() return
    ids, desc, valid = run.descriptors(0)
    for kw in (dict(), dict(max_distance=40, ratio=0.8, cross_check=False), dict(max_distance=30)):
        hits = run.query_keyframes(0, **kw)
        assert [hk for hk, _, _, _ in hits] == [0, 1]
        opts = dict(dict(max_distance=256, ratio=0.0, cross_check=True), **kw)
        for hk, ht, hn, pairs in hits:
            n, want = _pairs_numpy(ids, desc, valid, run.keyframe(0, hk), **opts)
            assert ht == kept[hk][0] and hn == n and np.array_equal(pairs, want), (kw, hk)
    counts = [hn for _, _, hn, _ in run.query_keyframes(0)]
    assert max(counts) >= 3
    # min_matches filters
    assert [hk for hk, _, hn, _ in run.query_keyframes(0, min_matches=min(counts) + 1)] == [k for k, n in enumerate(counts) if n >= min(counts) + 1]
    assert run.query_keyframes(0, min_matches=max(counts) + 1) == []
    assert [hk for hk, _, _, _ in run.query_keyframes(1)] == [0]
    with pytest.raises(R.MskfError):
        run.query_keyframes(0, max_distance=300)
    with pytest.raises(IndexError):
        run.keyframe(0, 2)
    # clear_keyframes empties: one stream, then all
    run.clear_keyframes(0)
    assert run.num_keyframes(0) == 0 and run.num_keyframes(1) == 1 and run.query_keyframes(0) == []
    run.clear_keyframes()
    assert run.num_keyframes(1) == 0
    # descriptors off: add_keyframe raises
    run.set_descriptors(False, stream=1)
    with pytest.raises(R.MskfError):
        run.add_keyframe(1)
    assert run.add_keyframe(0) == 0
    run.close()
