"""Numpy restatement of the ZNCC patch check ("Patch check"; csrc/hip/fe_patch.h on the device and in the C ABI),
written from the contract and not from the header:

    coordinate  x = min(max(x, 0), W - 1) in float32 (a NaN becomes 0); ix = floor(x); ax = (int)((x - ix) * 32) in float32;
    sample      at (dx, dy): the pixels at columns ix + dx, ix + dx + 1 and rows iy + dy, iy + dy + 1, indices clamped to the image;
                s = (32-ax)(32-ay) I00 + ax (32-ay) I10 + (32-ax) ay I01 + ax ay I11; v = (s + 128) >> 8;
    sums        SA, SB, SAA, SBB, SAB over the (2 half + 1)^2 = N samples; num = N SAB - SA SB, va = N SAA - SA^2, vb = N SBB - SB^2;
    decision    va == vb == 0 passes; else num > 0 and (double)num (double)num >= thr2 ((double)va (double)vb), thr2 = (double)t (double)t;
    gate        temporal (mode bit 1, do_temporal, status bit 0): in_pts in prev0 against out0 in curr0; a failing point gets
                status 0, out1 = und0 = und1 = 0, out0 kept.  Then stereo (mode bit 2, status bit 1): out0 in curr0 against out1
                in curr1; a failing point loses bit 1 and nothing else.

Everything is vectorised over points.  `mutate` plants one deliberate mistake (MUTATIONS) for the tests that show the cases
would see it."""
import numpy as np

MIN_HALF, MAX_HALF = 2, 7
TEMPORAL, STEREO = 1, 2
MUTATIONS = [
    "no_round",            # v = s >> 8, the + 128 dropped
    "no_clamp",            # indices outside the image wrap around instead of being clamped
    "gt",                  # > for >= in the decision
    "no_num_positive",     # num > 0 dropped: an inverted patch passes
    "n_even",              # N taken as (2 half)^2 in num, va and vb
    "round_frac",          # ax rounded to the nearest 32nd instead of truncated
]


def thr2(t):
    t = np.float64(np.float32(t))
    return t * t


def coord(x, size, mutate=None):
    """(ix, ax) int64 arrays of float32 coordinates in an image `size` pixels wide (or high)."""
    x = np.atleast_1d(np.asarray(x, np.float32)).copy()
    x[np.isnan(x)] = 0
    x = np.minimum(np.maximum(x, np.float32(0)), np.float32(size - 1)).astype(np.float32)
    fx = np.floor(x).astype(np.float32)
    frac = ((x - fx).astype(np.float32) * np.float32(32)).astype(np.float32)
    if mutate == "round_frac":
        frac = np.rint(frac)
    return fx.astype(np.int64), frac.astype(np.int64)


def samples(img, x, y, half, mutate=None):
    """(n, 2 half + 1, 2 half + 1) int64: the samples of the patches around the points (x, y), rows = dy."""
    img = np.asarray(img, np.uint8)
    h, w = img.shape
    ix, ax = coord(x, w, mutate)
    iy, ay = coord(y, h, mutate)
    d = np.arange(-half, half + 1)
    cx0, cx1 = ix[:, None] + d[None, :], ix[:, None] + d[None, :] + 1          # (n, side)
    cy0, cy1 = iy[:, None] + d[None, :], iy[:, None] + d[None, :] + 1
    if mutate == "no_clamp":
        cx0, cx1, cy0, cy1 = cx0 % w, cx1 % w, cy0 % h, cy1 % h
    else:
        cx0, cx1, cy0, cy1 = np.clip(cx0, 0, w - 1), np.clip(cx1, 0, w - 1), np.clip(cy0, 0, h - 1), np.clip(cy1, 0, h - 1)
    I = img.astype(np.int64)
    i00, i10 = I[cy0[:, :, None], cx0[:, None, :]], I[cy0[:, :, None], cx1[:, None, :]]
    i01, i11 = I[cy1[:, :, None], cx0[:, None, :]], I[cy1[:, :, None], cx1[:, None, :]]
    ax, ay = ax[:, None, None], ay[:, None, None]
    s = (32 - ax) * (32 - ay) * i00 + ax * (32 - ay) * i10 + (32 - ax) * ay * i01 + ax * ay * i11
    return (s + (0 if mutate == "no_round" else 128)) >> 8


def sums(img_a, xa, ya, img_b, xb, yb, half, mutate=None):
    """(n, 5) int64: SA, SB, SAA, SBB, SAB of the patches around (xa, ya) in img_a and (xb, yb) in img_b."""
    n_samples = (2 * half + 1) ** 2
    a = samples(img_a, xa, ya, half, mutate).reshape(-1, n_samples)
    b = samples(img_b, xb, yb, half, mutate).reshape(-1, n_samples)
    return np.stack([a.sum(1), b.sum(1), (a * a).sum(1), (b * b).sum(1), (a * b).sum(1)], 1)


def terms(s, half, mutate=None):
    """(num, va, vb) int64 of sums()."""
    n = (2 * half) ** 2 if mutate == "n_even" else (2 * half + 1) ** 2
    s = np.asarray(s, np.int64)
    return n * s[:, 4] - s[:, 0] * s[:, 1], n * s[:, 2] - s[:, 0] * s[:, 0], n * s[:, 3] - s[:, 1] * s[:, 1]


def decide(s, half, t2, mutate=None):
    """bool array: the points whose sums pass at the squared threshold t2."""
    num, va, vb = terms(s, half, mutate)
    nd, vd = num.astype(np.float64), va.astype(np.float64) * vb.astype(np.float64)
    lhs, rhs = nd * nd, np.float64(t2) * vd
    ok = (lhs > rhs) if mutate == "gt" else (lhs >= rhs)
    if mutate != "no_num_positive":
        ok &= num > 0
    return ((va == 0) & (vb == 0)) | ok


def zncc(s, half):
    """float64, for choosing thresholds only: num / sqrt(va vb), 1 where both patches are flat, 0 where one is."""
    num, va, vb = (x.astype(np.float64) for x in terms(s, half))
    with np.errstate(divide="ignore", invalid="ignore"):
        z = num / np.sqrt(va * vb)
    return np.where((va == 0) & (vb == 0), 1.0, np.where((va == 0) | (vb == 0), 0.0, z))


def gate(prev0, curr0, curr1, mode, half, t_temporal, t_stereo, do_temporal, in_pts, out0, out1, und0, und1, status, mutate=None):
    """The point gate on (n, 2) float32 arrays and (n,) uint8 status.  Returns new copies (out0, out1, und0, und1, status)."""
    out0, out1, und0, und1 = (np.array(a, np.float32).reshape(-1, 2) for a in (out0, out1, und0, und1))
    status = np.array(status, np.uint8)
    n = len(status)
    lost = np.zeros(n, bool)
    if (mode & TEMPORAL) and do_temporal and n:
        pin = np.array(in_pts, np.float32).reshape(-1, 2)
        k = np.flatnonzero(status & 1)
        s = sums(prev0, pin[k, 0], pin[k, 1], curr0, out0[k, 0], out0[k, 1], half, mutate)
        lost[k] = ~decide(s, half, thr2(t_temporal), mutate)
    unmatched = np.zeros(n, bool)
    if (mode & STEREO) and n:
        k = np.flatnonzero(((status & 2) != 0) & ~lost)
        s = sums(curr0, out0[k, 0], out0[k, 1], curr1, out1[k, 0], out1[k, 1], half, mutate)
        unmatched[k] = ~decide(s, half, thr2(t_stereo), mutate)
    status[lost] = 0
    out1[lost] = 0
    und0[lost] = 0
    und1[lost] = 0
    status[unmatched] &= np.uint8(0xFD)
    return out0, out1, und0, und1, status
