"""k_fe_book on the device against the host run of the same source (csrc/hip/fe_book.h), at its edges.

The cases are those of tests/cpp/fe_book_device_cases.cpp; tests/test_fe_book_cases.py shows on the CPU that each equals the
reference flow and reaches the edge it is named for.  Here every case runs through the library's own launch entry
(fe_launch_book, one workgroup per book) on an arena in device memory, and after each of the two launches of every frame the
WHOLE arena - tracked list, detections, candidates and their indices, cand_off / cand_cnt / cell_count, the published grid
and the export block, FeBookState, the RANSAC scratch and draw counter, and the canary tail of every array - must equal the
host arena byte for byte.  Everything is integer or float-exact: there is no tolerance.  What only the device has is what
this sees: the barriers, the items of a phase running side by side, the slots FB_INC hands out in any order, the shuffle
scan and its carry across passes of 256, the double / float arithmetic of fb_two_point_ransac as compiled for the GPU, and
the dynamic LDS above 64 KiB.

The descriptor self-check of the helper runs before every launch (a descriptor that fails it is never launched); after every
launch the stream is synchronised and hipGetLastError read, and after a HIP error nothing further is launched.

The last test drives the 8-bit push generation of the detector's cell keys through its wrap (push_gen_tag, mskf_capi_fe.cpp).
"""
import ctypes as C

import numpy as np
import pytest

from msckf_stereo_c_amd import capi
from msckf_stereo_c_amd import runner as R
from msckf_stereo_c_amd.ctypes_types import default_ekf_cfg, default_fe_cfg

import fe_book_cases as F
from hip_runtime import Hip
from test_fe_book_cases import SETS

pytestmark = pytest.mark.gpu

KiB = 1024
_HIP_ERRORS = []        # after a HIP error no test of this module launches anything


def _entry(ctx):
    L = ctx.L
    L.fe_book_lds_budget.argtypes = []
    L.fe_book_lds_budget.restype = C.c_size_t
    L.fe_launch_book.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_size_t, C.c_void_p]
    L.fe_launch_book.restype = None
    return L


def _launch(ctx, hip, desc, n, which, scratch_bytes):
    assert not _HIP_ERRORS, "an earlier launch ended with a HIP error: %s" % _HIP_ERRORS
    L = _entry(ctx)
    try:
        L.fe_launch_book(desc, n, which, scratch_bytes, ctx.hip_stream())
        ctx.sync()
        err = hip.last_error()
        assert err == 0, "hipGetLastError %d after k_fe_book(which = %d)" % (err, which)
    except BaseException as e:
        _HIP_ERRORS.append(repr(e))
        raise


def _run_books(ctx, hip, runs, scratch_bytes=None, n_frames=None):
    """The cases `runs` as the books of ONE launch per frame and half: per frame upload every book's descriptor and inputs,
    launch fe_book1, compare every whole arena with its host run, upload the candidates' results, launch fe_book2, compare.
    Returns, per book, the arenas read back (two per frame)."""
    budget = _entry(ctx).fe_book_lds_budget()
    assert budget == 150 * KiB
    n = len(runs)
    dsz = runs[0].desc_size
    scratch = max(r.scratch_bytes for r in runs) if scratch_bytes is None else scratch_bytes      # (as mskf_fe_frame_batch: the largest)
    assert max(r.scratch_bytes for r in runs) <= scratch <= budget
    frames = min(r.n_frames for r in runs) if n_frames is None else n_frames
    arenas = [hip.alloc(r.size, False) for r in runs]
    descs = hip.alloc(dsz * n, False)
    for r, a in zip(runs, arenas):
        hip.put(a, r.initial)
    back = [[] for _ in runs]
    busy = [0 for _ in runs]            # launches whose host run changes the arena
    for f in range(frames):
        for half in (0, 1):
            for k, (r, a) in enumerate(zip(runs, arenas)):
                d = r.desc(f, a)
                bad = r.check_desc(f, d, a, r.size, budget)
                assert bad is None, (r.name, f, bad)
                hip.put(descs + k * dsz, d)
                lo, hi = r.ranges[half]
                before = r.snapshot(f, 2 * half)
                hip.put(a + lo, np.ascontiguousarray(before[lo:hi]))
                busy[k] += 0 if np.array_equal(before, r.snapshot(f, 2 * half + 1)) else 1
            _launch(ctx, hip, descs, n, half, scratch)
            for k, (r, a) in enumerate(zip(runs, arenas)):
                got = hip.get(a, r.size)
                diff = r.where(got, r.snapshot(f, 2 * half + 1))
                assert diff is None, "%s (book %d of %d) frame %d after fe_book%d: device != host at %s" % (r.name, k, n, f, half + 1, diff)
                back[k].append(got)
    # the launches had something to do: a kernel that wrote nothing could not have passed the comparisons
    assert all(b >= 2 * frames - 2 for b in busy), busy
    return back


@pytest.mark.parametrize("case_set", SETS)
def test_device_book_equals_host_book(gpu_ctx, case_set):
    """Every case of the set, one book per launch."""
    lib = F.lib()
    hip = Hip()
    try:
        for i in lib.of_set(case_set):
            r = lib.run(i)
            assert not r.error, (r.name, r.error)
            _run_books(gpu_ctx, hip, [r])
            if case_set == "lds":
                assert r.scratch_bytes > 64 * KiB
            r.close()
            hip.free()
    finally:
        gpu_ctx.sync()
        hip.free()


BATCH = ["crowded_tied_lifetimes", "n_prev_0", "grid_16_16", "ransac_clean_translation", "q7_333x251_3x7", "cand_all_pass"]


def test_six_different_books_in_one_launch(gpu_ctx):
    """Six books of different configurations and capacities as the workgroups of one launch, scratch_bytes the largest of
    them: every book's arena equals its host run (inside _run_books) and its own single-book launch."""
    lib = F.lib()
    hip = Hip()
    try:
        runs = [lib.run(lib.index(name)) for name in BATCH]
        assert len({(r.size, r.scratch_bytes) for r in runs}) >= 4
        together = _run_books(gpu_ctx, hip, runs)
        frames = len(together[0]) // 2
        assert frames >= 3
        for k, r in enumerate(runs):
            alone = _run_books(gpu_ctx, hip, [r], n_frames=frames)[0]
            for j, (x, y) in enumerate(zip(together[k], alone)):
                assert r.where(x, y) is None, (r.name, j, r.where(x, y))
            r.close()
    finally:
        gpu_ctx.sync()
        hip.free()


@pytest.mark.parametrize("name", ["cand_all_pass", "ransac_cam1_rejects", "lds_over_64k"])
def test_scratch_larger_than_the_books_own(gpu_ctx, name):
    """The same book launched with more dynamic LDS than it needs (as a small book beside a large one in a batch): the same
    bytes.  Nothing may depend on where the scratch ends."""
    lib = F.lib()
    hip = Hip()
    try:
        r = lib.run(lib.index(name))
        for scratch in (r.scratch_bytes + 1024, 150 * KiB):
            _run_books(gpu_ctx, hip, [r], scratch_bytes=scratch)         # (compares with the host run, which is what its own size gives)
            hip.free()
        r.close()
    finally:
        gpu_ctx.sync()
        hip.free()


# ------------------------------------------------------------------------------------------ detector key generations
def _textured(w, h, seed):
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 40, (h, w)).astype(np.uint8)
    for _ in range(12):                                    # bright blocks: corners the detector scores well above the threshold
        x, y = int(rng.integers(2, w - 12)), int(rng.integers(2, h - 12))
        img[y:y + 9, x:x + 9] = 200 + int(rng.integers(0, 50))
    return img


def test_cell_key_generations_across_the_wrap(oracle):
    """The cell keys carry an 8-bit push generation and the key array is cleared only when fresh or when the tag wraps to 1.
    A context of its own, two streams of different sizes pushed alone and together in either order (their slices of the shared
    key array move), 260 pushes of images that cycle textured, flat, textured: after every push the maxima of every pushed
    stream equal the oracle's - in particular around pushes 254 .. 258, and a flat image after a textured one reads as no
    corner in any cell (a stale key must never pass for this push's)."""
    ctx = capi.Context(0)
    try:
        sizes = [(64, 64), (128, 96)]
        ss = [capi.Stream(ctx, oracle.euroc_calib(w, h), default_fe_cfg(), default_ekf_cfg()) for w, h in sizes]
        imgs = [[_textured(w, h, 1 + 10 * k), np.full((h, w), 90, np.uint8), _textured(w, h, 2 + 10 * k)] for k, (w, h) in enumerate(sizes)]
        want = [[oracle.cell_maxima(im) for im in three] for three in imgs]
        for three in want:
            assert (three[0]["score"] > 2560).sum() > 8 and (three[2]["score"] > 2560).sum() > 8 and not three[1]["score"].any()
        count = [0, 0]
        schedule = [[0], [1], [0, 1], [1, 0], [1], [0, 1], [0]]
        flat_after_textured = 0
        for push in range(1, 261):
            who = schedule[push % len(schedule)]
            kinds = [count[k] % 3 for k in who]
            if len(who) == 1:
                ss[who[0]].push_stereo(imgs[who[0]][kinds[0]], imgs[who[0]][kinds[0]])
            else:
                ctx.push_stereo_batch([ss[k] for k in who], [imgs[k][j] for k, j in zip(who, kinds)], [imgs[k][j] for k, j in zip(who, kinds)])
            for k, j in zip(who, kinds):
                got, ref = ss[k].cell_maxima(), want[k][j]
                for key in ("score", "x", "y"):
                    assert np.array_equal(got[key], ref[key]), (push, k, j, key)
                if j == 1:
                    assert not got["score"].any(), (push, k)
                    flat_after_textured += 1
                count[k] += 1
        assert flat_after_textured > 80
        for s in ss:
            s.close()
    finally:
        ctx.close()


def test_device_books_equal_host_books_across_the_wrap(oracle):
    """One stream through 259 frames with its books on the device (mskf_fe_frame_batch_*: fe_book1 trusts the generation the
    descriptor carries) and the same stream with its books on the host: identical grids and tracking info in the frames
    around the wrap of the 8-bit generation (pushes 254 .. 259)."""
    w, h = 188, 120
    fe, ekf = default_fe_cfg(), default_ekf_cfg(max_cam_state_size=10)
    syn = oracle.Synth(seed=0x5EED0091, width=w, height=h, n_static=1, n_loop=40)
    runs = []
    try:
        for host in (1, 0):
            R.set_fe_books_on_host(host)
            runs.append(R.Runner(syn.calib, fe, ekf, 1, 1))
        j = 0
        checked = 0
        for k in range(259):
            t_img = syn.frame_time(k)
            while True:
                s = syn.imu(j)
                j += 1
                for r in runs:
                    r.imu(0, s)
                if not (s.time_stamp <= t_img):
                    break
            a, b = syn.render(k)
            for host, r in zip((1, 0), runs):
                R.set_fe_books_on_host(host)
                r.step([a], [b], [t_img])
            if k >= 252 or k % 50 == 0:
                da, db = runs[0].dump(0), runs[1].dump(0)
                for x, y in zip(da[:4], db[:4]):
                    assert x.tobytes() == y.tobytes(), k
                assert bytes(da[4]) == bytes(db[4]), k
                assert len(da[0]) > 20, k
                checked += 1
        assert checked >= 12
        assert runs[1].num_device_frames(0) >= 250 and runs[0].num_device_frames(0) == 0
    finally:
        R.set_fe_books_on_host(-1)
        for r in runs:
            r.close()
