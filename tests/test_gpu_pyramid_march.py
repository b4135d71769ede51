"""k_pyr_down3 as a register / DPP row march: every level of both cameras against the oracle's pyr_down, byte for byte, at
the sizes where the march changes what it does.

A 16-lane strip owns 12 level-3 columns = 96 level-0 columns; a segment owns `seg3` level-3 rows = 8 * seg3 level-0 rows, with
seg3 chosen by the launcher (fe_launch_pyr_down3): at most 8 in a launch that fills the device, at most 4 in the small
launches of a test, the segments of a launch made equally long.  Images go through the C-ABI push where it accepts them
(64 x 64 and larger) and straight to the launch entry otherwise, which also takes jobs of different sizes in one launch.
The direct launches put guard bytes around every output level: a store outside a level shows."""
import ctypes as C

import numpy as np
import pytest

from msckf_stereo_c_amd import capi
from msckf_stereo_c_amd.ctypes_types import default_ekf_cfg, default_fe_cfg

from hip_runtime import Hip

pytestmark = pytest.mark.gpu

STRIP = 96          # level-0 columns a strip owns
GUARD = 64          # guard bytes in front of and behind every output level of a direct launch
_HIP_ERRORS = []    # after a HIP error no test of this module launches anything


class Pyr3Job(C.Structure):
    _fields_ = [("src", C.c_void_p), ("d1", C.c_void_p), ("d2", C.c_void_p), ("d3", C.c_void_p), ("w0", C.c_int), ("h0", C.c_int)]


def _dims(w, h):
    out = [(w, h)]
    for _ in range(3):
        w, h = (w + 1) // 2, (h + 1) // 2
        out.append((w, h))
    return out


def _seg3(n_jobs, max_w, max_h):
    """The launcher's choice of level-3 rows per segment."""
    w3, h3 = _dims(max_w, max_h)[3]
    strips = (w3 + 11) // 12
    target = 8
    while target > 4 and n_jobs * strips * ((h3 + target - 1) // target) // 4 < 2048:
        target //= 2
    segs = (h3 + target - 1) // target
    return (h3 + segs - 1) // segs


def _check_pushed(gpu_ctx, oracle, a, b, **push):
    h, w = a.shape[0], a.shape[1] if not push else push.pop("w")
    s = capi.Stream(gpu_ctx, oracle.euroc_calib(w, h), default_fe_cfg(), default_ekf_cfg())
    s.push_stereo(a, b, **push)
    for role, img in ((1, a), (2, b)):
        ref = oracle.build_pyramid(np.ascontiguousarray(img[:, :w]))
        for lvl in range(4):
            got = s.get_level(role, lvl)
            assert got.shape == ref[lvl].shape
            assert np.array_equal(got, ref[lvl]), (role, lvl)
    s.close()


def _random_pair(w, h):
    rng = np.random.default_rng(w * 1000 + h)
    return rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (h, w), dtype=np.uint8)


def _launch_direct(gpu_ctx, oracle, imgs, job_img=None):
    """One fe_launch_pyr_down3 over the images `imgs` (job k reads imgs[job_img[k]], every job writes levels of its own) and
    the comparison of every job's three levels, and of the guard bytes around them, with the oracle."""
    assert not _HIP_ERRORS, "an earlier launch ended with a HIP error: %s" % _HIP_ERRORS
    job_img = list(range(len(imgs))) if job_img is None else job_img
    hip = Hip()
    L = gpu_ctx.L
    L.fe_launch_pyr_down3.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.fe_launch_pyr_down3.restype = None
    try:
        src_off, n_src = [], 0
        for img in imgs:
            src_off.append(n_src)
            n_src += (img.size + 15) // 16 * 16
        out_off, n_out = [], 0
        for k in job_img:
            offs = []
            for (w, h) in _dims(imgs[k].shape[1], imgs[k].shape[0])[1:]:
                offs.append(n_out + GUARD)
                n_out += GUARD + w * h
            out_off.append(offs)
        n_out += GUARD
        host_src = np.zeros(n_src, np.uint8)
        for img, o in zip(imgs, src_off):
            host_src[o:o + img.size] = img.reshape(-1)
        d_src, d_out = hip.alloc(n_src, False), hip.alloc(n_out, False)
        hip.put(d_src, host_src)
        hip.put(d_out, np.full(n_out, 0xA5, np.uint8))
        jobs = (Pyr3Job * len(job_img))()
        for j, k in enumerate(job_img):
            jobs[j].src = d_src + src_off[k]
            jobs[j].d1, jobs[j].d2, jobs[j].d3 = (d_out + o for o in out_off[j])
            jobs[j].h0, jobs[j].w0 = imgs[k].shape
        raw = np.frombuffer(bytes(jobs), np.uint8).copy()
        d_jobs = hip.alloc(raw.size, False)
        hip.put(d_jobs, raw)
        L.fe_launch_pyr_down3(d_jobs, len(job_img), max(i.shape[1] for i in imgs), max(i.shape[0] for i in imgs), gpu_ctx.hip_stream())
        gpu_ctx.sync()
        err = hip.last_error()
        assert err == 0, "hipGetLastError %d after k_pyr_down3" % err
        got = hip.get(d_out, n_out)
    except BaseException as e:
        _HIP_ERRORS.append(repr(e))
        raise
    finally:
        hip.free()
    refs = {k: oracle.build_pyramid(imgs[k]) for k in set(job_img)}
    written = np.zeros(n_out, bool)
    for j, k in enumerate(job_img):
        for lvl, o in zip((1, 2, 3), out_off[j]):
            ref = refs[k][lvl]
            assert np.array_equal(got[o:o + ref.size].reshape(ref.shape), ref), (j, imgs[k].shape, lvl)
            written[o:o + ref.size] = True
    assert np.all(got[~written] == 0xA5), "a store outside the levels"


@pytest.mark.parametrize("w", [STRIP, STRIP - 1, STRIP + 1, 2 * STRIP, 2 * STRIP - 1, 2 * STRIP + 1])
def test_widths_around_a_strip(gpu_ctx, oracle, w):
    """The last owner lane of a strip holds the image's last column, the one before it, or the first lane of the next strip
    does; the same around two strips."""
    _check_pushed(gpu_ctx, oracle, *_random_pair(w, 72))


@pytest.mark.parametrize("h", [64, 65, 71, 72, 73, 127, 128, 129])
def test_heights_around_a_segment(gpu_ctx, oracle, h):
    """A two-image launch of these heights is cut into segments of 3 or 4 level-3 rows (24 or 32 level-0 rows): heights that
    are a whole number of segments, one row less and one more, at one width inside a strip."""
    assert _seg3(2, 80, h) in (3, 4)
    _check_pushed(gpu_ctx, oracle, *_random_pair(80, h))


@pytest.mark.parametrize("h", [32, 31, 33])
def test_heights_around_one_segment(gpu_ctx, oracle, h):
    """Exactly one segment of four level-3 rows, one level-0 row less, one more (a second segment)."""
    rng = np.random.default_rng(h)
    _launch_direct(gpu_ctx, oracle, [rng.integers(0, 256, (h, 40), dtype=np.uint8)])


@pytest.mark.parametrize("w,h", [(9, 7), (16, 16), (17, 33), (64, 64), (8, 1), (3, 3), (1, 8), (5, 2), (2, 5)])
def test_tiny_images(gpu_ctx, oracle, w, h):
    """Every level reflects on both sides at once, levels of one or two columns / rows included; 64 x 64 is the smallest
    image the C-ABI accepts, the others go straight to the launch entry."""
    if w >= 64 and h >= 64:
        _check_pushed(gpu_ctx, oracle, *_random_pair(w, h))
    else:
        _launch_direct(gpu_ctx, oracle, list(_random_pair(w, h)))


@pytest.mark.parametrize("w,h", [(1280, 18), (18, 720)])
def test_thin_images(gpu_ctx, oracle, w, h):
    _launch_direct(gpu_ctx, oracle, list(_random_pair(w, h)))


@pytest.mark.parametrize("w,h", [(753, 481), (750, 478), (745, 473), (747, 475), (749, 477), (751, 479), (756, 484)])
def test_odd_at_every_level(gpu_ctx, oracle, w, h):
    """(w, w1, w2) and (h, h1, h2) odd / even in every combination: 753 -> 377 -> 189 (odd, odd, odd), 750 -> 375 -> 188,
    745 -> 373 -> 187, 747 -> 374 -> 187, 749 -> 375 -> 188, 751 -> 376 -> 188, 756 -> 378 -> 189, and the heights alike."""
    _check_pushed(gpu_ctx, oracle, *_random_pair(w, h))


def test_mixed_launch(gpu_ctx, oracle):
    """Jobs of different sizes in one launch whose job count is no multiple of 8.  The launch is cut for its largest image
    (200 x 64: three strips, two segments of four level-3 rows); the 70 x 33 image's second segment owns a single level-3 row,
    other images end inside the first strip or the first segment, one is wider than it is cut for in neither direction."""
    assert _seg3(11, 200, 64) == 4
    shapes = [(200, 64), (70, 33), (9, 7), (96, 32), (97, 40), (16, 16), (200, 8), (8, 64), (191, 63), (33, 17), (120, 57)]
    rng = np.random.default_rng(11)
    _launch_direct(gpu_ctx, oracle, [rng.integers(0, 256, (h, w), dtype=np.uint8) for (w, h) in shapes])


def test_device_filling_launch(gpu_ctx, oracle):
    """Enough jobs that the launcher keeps its longest segments (8 level-3 rows, 88 level-0 rows marched per job): 1024 jobs
    over 32 different images of 16 x 1024."""
    assert _seg3(1024, 16, 1024) == 8
    rng = np.random.default_rng(1024)
    imgs = [rng.integers(0, 256, (1024, 16), dtype=np.uint8) for _ in range(32)]
    _launch_direct(gpu_ctx, oracle, imgs, job_img=[j % 32 for j in range(1024)])


def test_pitched_push(gpu_ctx, oracle):
    """A pitched host-image push (rows 13 bytes longer than the image) of a size that is odd at every level."""
    w, h, pitch = 333, 251, 346
    rng = np.random.default_rng(346)
    a = rng.integers(0, 256, (h, pitch), dtype=np.uint8)
    b = rng.integers(0, 256, (h, pitch), dtype=np.uint8)
    _check_pushed(gpu_ctx, oracle, a, b, w=w, pitch=pitch)
