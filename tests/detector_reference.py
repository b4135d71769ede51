"""Numpy restatement of the corner detector (k_detect_cells on the device, CornerDetector::cell_maxima in the
oracle), written from the definition and not from either: int64 arithmetic, math.isqrt.

    dx = I[y, x + 1] - I[y, x - 1],  dy = I[y + 1, x] - I[y - 1, x]                       (central differences)
    a, b, c = sums of dx dx, dx dy, dy dy over the rows y - 4 .. y + 3 and the columns x - 4 .. x + 3
    score   = a + c - isqrt((a - c)^2 + 4 b^2)      for 8 <= x < W - 8 and 8 <= y < H - 8, zero outside
    a cell is cell_w x cell_h pixels (the ceil of the image size over the grid unless given); it records its largest score
    above `floor`, the first pixel in row-major order among equals.

On the device the maxima are merged as 64-bit keys  gen (8 bits) | score (24 bits) | ~order (32 bits), order = the row-major
position inside the cell: keys_of / merge_keys restate that, the GPU tests decode what the kernel left.

`mutate` plants one deliberate mistake (MUTATIONS) for the tests that show the case set would see it in the kernel."""
import math

import numpy as np

BORDER = 8          # no score closer to the image edge
STRIP_COLS = 56     # output columns of a 16-lane strip of the kernel's march
RESULT = np.dtype([("score", "<i8"), ("x", "<i8"), ("y", "<i8"), ("has", "?")])

MUTATIONS = [
    "tie_last",                 # ties go to the last pixel in row-major order
    "ge_floor",                 # score >= floor is recorded
    "isqrt_up",                 # the square root is rounded up
    "isqrt_square_low",         # the square root is one too small on perfect squares, zero included
    "drop_cell_last_row",       # the last row of every cell is never scored
    "drop_seg32_last_row",      # the last row of every 32-row segment is never scored
    "drop_seg64_last_row",      # ... of every 64-row segment
    "drop_seg128_last_row",     # ... of every 128-row segment
    "drop_strip_col57",         # the 57th output column of a strip (the first of the next one) is never scored
    "drop_col_w9",              # column W - 9, the last scored one
    "drop_row_h9",              # row H - 9, the last scored one
    "mask23",                   # the score is masked to 23 bits (no image can show it: see max_score)
    "mask22",                   # the score is masked to 22 bits
    "stale_wins",               # a key of an older generation is kept when its score is larger
]
SCORE_MUTATIONS = ["isqrt_up", "isqrt_square_low", "mask23", "mask22"]      # the ones that change the score map itself


def max_score():
    """The largest score any image has: a + c with every one of the 64 differences at 255 in both directions and a root of 0."""
    return 2 * 64 * 255 * 255


def seg_rows(n_streams, max_w, max_h):
    """The rows of a segment as fe_launch_detect chooses them for a launch cut for max_w x max_h."""
    strips, rows = (max_w - 2 * BORDER + STRIP_COLS - 1) // STRIP_COLS, max_h - 2 * BORDER
    assert strips > 0 and rows > 0
    s = 32
    while s < 128 and n_streams * strips * ((rows + s - 1) // s) // 4 > 32768:
        s *= 2
    return s


def _box8(p):
    """Sums of p over the rows y - 4 .. y + 3 and the columns x - 4 .. x + 3, where that window lies inside p (zero elsewhere)."""
    h, w = p.shape
    q = np.zeros((h + 1, w + 1), np.int64)
    q[1:, 1:] = p.cumsum(0).cumsum(1)
    out = np.zeros((h, w), np.int64)
    out[4:h - 3, 4:w - 3] = q[8:, 8:] - q[:-8, 8:] - q[8:, :-8] + q[:-8, :-8]
    return out


def box_sums(img):
    """a, b, c at every pixel (meaningful where valid_mask holds)."""
    i = np.asarray(img).astype(np.int64)
    dx, dy = np.zeros_like(i), np.zeros_like(i)
    dx[:, 1:-1] = i[:, 2:] - i[:, :-2]
    dy[1:-1, :] = i[2:, :] - i[:-2, :]
    return _box8(dx * dx), _box8(dx * dy), _box8(dy * dy)


def valid_mask(w, h):
    m = np.zeros((h, w), bool)
    m[BORDER:h - BORDER, BORDER:w - BORDER] = True
    return m


def _isqrt(v, mutate):
    r = math.isqrt(v)
    if mutate == "isqrt_up" and r * r != v:
        r += 1
    if mutate == "isqrt_square_low" and r * r == v:
        r -= 1
    return r


def score_map(img, mutate=None):
    """(h, w) int64 scores, zero outside the border."""
    h, w = np.asarray(img).shape
    assert w > 2 * BORDER and h > 2 * BORDER
    a, b, c = box_sums(img)
    disc = (a - c) * (a - c) + 4 * b * b
    root = np.array([_isqrt(int(v), mutate) for v in disc.ravel()], np.int64).reshape(h, w)
    score = np.where(valid_mask(w, h), a + c - root, 0)
    if mutate in ("mask23", "mask22"):
        score &= (1 << int(mutate[4:])) - 1
    return score


def ceil_cells(w, h, det_rows, det_cols):
    return (w + det_cols - 1) // det_cols, (h + det_rows - 1) // det_rows


def reduce_cells(score, det_rows, det_cols, cell_w, cell_h, floor=0, mutate=None):
    """Per-cell maxima of a score map: RESULT records in cell order."""
    h, w = score.shape
    assert cell_w * det_cols >= w and cell_h * det_rows >= h
    yy, xx = np.mgrid[0:h, 0:w]
    keep = valid_mask(w, h)
    if mutate == "drop_cell_last_row":
        keep &= yy % cell_h != cell_h - 1
    if mutate in ("drop_seg32_last_row", "drop_seg64_last_row", "drop_seg128_last_row"):
        s = int(mutate[8:-9])
        keep &= (yy - BORDER) % s != s - 1
    if mutate == "drop_strip_col57":
        keep &= ~(((xx - BORDER) % STRIP_COLS == 0) & (xx > BORDER))
    if mutate == "drop_col_w9":
        keep &= xx != w - BORDER - 1
    if mutate == "drop_row_h9":
        keep &= yy != h - BORDER - 1
    keep &= (score >= floor) if mutate == "ge_floor" else (score > floor)
    cell = (yy // cell_h) * det_cols + xx // cell_w
    order = (yy % cell_h) * cell_w + xx % cell_w
    rank = score * (1 << 32) + (order if mutate == "tie_last" else (1 << 32) - 1 - order)     # score < 2^24: fits an int64
    best = np.full(det_rows * det_cols, -1, np.int64)
    np.maximum.at(best, cell[keep], rank[keep])
    out = np.zeros(det_rows * det_cols, RESULT)
    has = best >= 0
    order = np.where(has, best & 0xFFFFFFFF, 0)
    if mutate != "tie_last":
        order = np.where(has, 0xFFFFFFFF - order, 0)
    cells = np.arange(det_rows * det_cols)
    out["has"] = has
    out["score"] = np.where(has, best >> 32, 0)
    out["x"] = np.where(has, (cells % det_cols) * cell_w + order % cell_w, 0)
    out["y"] = np.where(has, (cells // det_cols) * cell_h + order // cell_w, 0)
    return out


def cell_maxima(img, det_rows, det_cols, floor=0, cell_w=None, cell_h=None, mutate=None):
    h, w = np.asarray(img).shape
    cw, ch = ceil_cells(w, h, det_rows, det_cols)
    return reduce_cells(score_map(img, mutate), det_rows, det_cols, cell_w or cw, cell_h or ch, floor, mutate)


def keys_of(res, det_cols, cell_w, cell_h, gen):
    """The keys a launch of generation `gen` sends for the RESULT records `res` (0: none for that cell)."""
    cells = np.arange(len(res))
    order = (res["y"] - (cells // det_cols) * cell_h) * cell_w + (res["x"] - (cells % det_cols) * cell_w)
    k = (np.uint64(gen) << np.uint64(56)) | (res["score"].astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - order.astype(np.uint64))
    return np.where(res["has"], k, np.uint64(0))


def merge_keys(before, sent, mutate=None):
    """The key array after the launch: the larger of what was there and what was sent, as unsigned 64-bit numbers."""
    before, sent = np.asarray(before, np.uint64), np.asarray(sent, np.uint64)
    if mutate == "stale_wins":
        low = np.uint64((1 << 56) - 1)
        return np.where((sent & low) > (before & low), sent, before)
    return np.maximum(before, sent)
