"""Restatement of the forward-backward check ("Forward-backward check"; csrc/hip/fe_fb.h and k_fb_points on the
device), written from the contract and not from the header:

    backward    temporal: oracle.lk_track(A = curr0, B = prev0, template at out0, initial guess in_pts), compared with in_pts;
                stereo:   oracle.lk_track(A = curr1, B = curr0, template at out1, initial guess out0), compared with out0.
                (oracle.lk_track is the CPU function the GPU tests pin l4_track to, bit for bit, all four pyramid levels.)
    fb_pass     dx = bx - ox, dy = by - oy; st != 0 and dx dx + dy dy <= thr2, every operation rounded to float32; a NaN fails;
                thr2 = t t in float32.
    gate        temporal (mode bit 1, do_temporal, status bit 0): a failing point gets status 0, out1 = und0 = und1 = 0, out0
                kept.  Then stereo (mode bit 2, status bit 1, not lost): a failing point loses bit 1 and nothing else.

Everything is vectorised over points.  `mutate` plants one deliberate mistake (MUTATIONS) for the tests that show the cases
would see it."""
import numpy as np

TEMPORAL, STEREO = 1, 2
MAX_ERROR = 64.0
MUTATIONS = [
    "lt",                  # < for <= in the decision
    "no_status",           # the backward track's status ignored
    "double",              # the distance formed in double precision
    "wrong_origin",        # the stereo half compares with the cam1 point the template was taken at, not with out0
]


def thr2(t):
    t = np.float32(t)
    return np.float32(t * t)


def fb_pass(bx, by, ox, oy, st, t2, mutate=None):
    """bool array: the points whose backward track (bx, by, st) returns to (ox, oy) within the squared threshold t2."""
    bx, by, ox, oy = (np.atleast_1d(np.asarray(v, np.float32)) for v in (bx, by, ox, oy))
    st = np.atleast_1d(np.asarray(st))
    with np.errstate(invalid="ignore", over="ignore"):
        if mutate == "double":
            dx, dy = bx.astype(np.float64) - ox.astype(np.float64), by.astype(np.float64) - oy.astype(np.float64)
            d2 = dx * dx + dy * dy
            t2 = np.float64(np.float32(t2))
        else:
            dx, dy = (bx - ox).astype(np.float32), (by - oy).astype(np.float32)
            d2 = ((dx * dx).astype(np.float32) + (dy * dy).astype(np.float32)).astype(np.float32)
            t2 = np.float32(t2)
        ok = (d2 < t2) if mutate == "lt" else (d2 <= t2)
    if mutate != "no_status":
        ok = ok & (st != 0)
    return ok


def _lk(img_a, img_b, pts_a, guess):
    from oracle import oracle_py
    return oracle_py.lk_track(img_a, img_b, pts_a, guess)


def gate(prev0, curr0, curr1, mode, thr_t, thr_s, do_temporal, in_pts, out0, out1, und0, und1, status, mutate=None):
    """The point gate on (n, 2) float32 arrays and (n,) uint8 status.  Returns new copies (out0, out1, und0, und1, status)."""
    out0, out1, und0, und1 = (np.array(a, np.float32).reshape(-1, 2) for a in (out0, out1, und0, und1))
    status = np.array(status, np.uint8)
    n = len(status)
    lost = np.zeros(n, bool)
    if (mode & TEMPORAL) and do_temporal and n:
        pin = np.array(in_pts, np.float32).reshape(-1, 2)
        k = np.flatnonzero(status & 1)
        if len(k):
            back, st = _lk(curr0, prev0, out0[k], pin[k])
            lost[k] = ~fb_pass(back[:, 0], back[:, 1], pin[k, 0], pin[k, 1], st, thr2(thr_t), mutate)
    unmatched = np.zeros(n, bool)
    if (mode & STEREO) and n:
        k = np.flatnonzero(((status & 2) != 0) & ~lost)
        if len(k):
            back, st = _lk(curr1, curr0, out1[k], out0[k])
            origin = out1[k] if mutate == "wrong_origin" else out0[k]
            unmatched[k] = ~fb_pass(back[:, 0], back[:, 1], origin[:, 0], origin[:, 1], st, thr2(thr_s), mutate)
    status[lost] = 0
    out1[lost] = 0
    und0[lost] = 0
    und1[lost] = 0
    status[unmatched] &= np.uint8(0xFD)
    return out0, out1, und0, und1, status


def round_trip(img_a, img_b, pts_a, origin):
    """(error in pixels float64, status) of the backward track of pts_a in img_a into img_b from `origin`: for choosing scenes."""
    back, st = _lk(img_a, img_b, pts_a, origin)
    d = back.astype(np.float64) - np.asarray(origin, np.float32).reshape(-1, 2).astype(np.float64)
    return np.hypot(d[:, 0], d[:, 1]), st
