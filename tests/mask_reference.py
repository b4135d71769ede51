"""Numpy restatement of the image masks ("Image masks"; csrc/hip/fe_mask.h on the device and in the C ABI), written
from the contract and not from the header:

    input    an 8-bit plane, a pixel != 0 is usable;
    erode    a pixel stays usable iff every pixel of the image within Chebyshev distance `margin` is non-zero (pixels outside the
             image count as usable);
    pack     32-bit words, (W + 31) // 32 per row, pixel x is bit x & 31 of word x >> 5, padding bits 0;
    pixel    of a point: (int)(x + 0.5f), float32 addition then truncation;
    gate     status bit 0 and a clear mask0 bit under out0: status 0, out1 = und0 = und1 = 0, out0 kept; else status bit 1 and a
             clear mask1 bit under out1: bit 1 cleared, nothing else;
    detector the per-cell reduction over the score map with the masked-out pixels' scores set to 0.

`mutate` plants one deliberate mistake (MUTATIONS) for the tests that show the cases would see it."""
import numpy as np

import detector_reference as DR

MAX_MARGIN = 64
MUTATIONS = [
    "margin_minus_one",         # the erosion reaches one pixel less far
    "margin_plus_one",          # ... one pixel further
    "msb_first",                # pixel x is bit 31 - (x & 31) of its word
    "truncate",                 # the pixel of a point is (int)x, without the + 0.5
    "mask1_clears_bit0",        # a clear mask1 bit loses the whole point
    "mask0_keeps_und0",         # a point lost to mask0 keeps und0
    "outside_masked",           # the erosion treats pixels outside the image as masked out
]


def usable_of(mask):
    return np.asarray(mask) != 0


def erode(mask, margin, mutate=None):
    """(h, w) bool: the usable set after the erosion by `margin`."""
    u = usable_of(mask)
    m = margin + {"margin_minus_one": -1, "margin_plus_one": 1}.get(mutate, 0)
    if m <= 0:
        return u.copy()
    h, w = u.shape
    pad = np.full((h + 2 * m, w + 2 * m), mutate != "outside_masked")
    pad[m:m + h, m:m + w] = u
    rows = np.full((h, w + 2 * m), True)      # (a square window is separable: the rows of the window first)
    for dy in range(2 * m + 1):
        rows &= pad[dy:dy + h, :]
    out = np.ones((h, w), bool)
    for dx in range(2 * m + 1):
        out &= rows[:, dx:dx + w]
    return out


def pitch_words(w):
    return (w + 31) // 32


def pack(usable, mutate=None):
    """(h, pitch_words(w)) uint32 bit plane of a bool plane."""
    u = np.asarray(usable, bool)
    h, w = u.shape
    pw = pitch_words(w)
    bits = np.zeros((h, pw * 32), np.uint64)
    bits[:, :w] = u
    sh = np.arange(32, dtype=np.uint64)
    if mutate == "msb_first":
        sh = np.uint64(31) - sh
    return (bits.reshape(h, pw, 32) << sh).sum(2).astype(np.uint32)


def lookup(words, w, h, px, py):
    """The bit of pixel (px, py) of a packed plane; outside the image: usable."""
    px, py = np.asarray(px, np.int64), np.asarray(py, np.int64)
    inside = (px >= 0) & (py >= 0) & (px < w) & (py < h)
    x, y = np.clip(px, 0, w - 1), np.clip(py, 0, h - 1)
    bit = (words[y, x >> 5] >> (x & 31).astype(np.uint32)) & np.uint32(1)
    return np.where(inside, bit != 0, True)


def pixel(v, mutate=None):
    """The pixel coordinate of float32 coordinates."""
    v = np.asarray(v, np.float32)
    if mutate == "truncate":
        return v.astype(np.int32)
    return (v + np.float32(0.5)).astype(np.float32).astype(np.int32)


def gate(mask0, mask1, w, h, out0, out1, und0, und1, status, mutate=None):
    """The point gate on (n, 2) float32 arrays and (n,) uint8 status; mask0 / mask1: packed planes or None.  Returns new copies
    (out0, out1, und0, und1, status)."""
    out0, out1, und0, und1 = (np.array(a, np.float32).reshape(-1, 2) for a in (out0, out1, und0, und1))
    status = np.array(status, np.uint8)
    n = len(status)
    lost = np.zeros(n, bool)
    if mask0 is not None:
        lost = ((status & 1) != 0) & ~lookup(mask0, w, h, pixel(out0[:, 0], mutate), pixel(out0[:, 1], mutate))
    unmatched = np.zeros(n, bool)
    if mask1 is not None:
        unmatched = ~lost & ((status & 2) != 0) & ~lookup(mask1, w, h, pixel(out1[:, 0], mutate), pixel(out1[:, 1], mutate))
    if mutate == "mask1_clears_bit0":
        lost, unmatched = lost | unmatched, np.zeros(n, bool)
    status[lost] = 0
    out1[lost] = 0
    und1[lost] = 0
    if mutate != "mask0_keeps_und0":
        und0[lost] = 0
    status[unmatched] &= np.uint8(0xFD)
    return out0, out1, und0, und1, status


def masked_cell_maxima(score, usable, det_rows, det_cols, cell_w, cell_h, floor=0):
    """detector_reference.RESULT records: the per-cell maxima of a score map (detector_reference.score_map) over the usable pixels."""
    return DR.reduce_cells(np.where(np.asarray(usable, bool), score, 0), det_rows, det_cols, cell_w, cell_h, floor)
