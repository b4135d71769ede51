"""The images, sizes and grids the detector kernel is driven with (tests/test_gpu_detector_edges.py), by name, and what the
oracle says about each.  tests/test_detector_cases.py shows on the CPU that the set is alive and that each mistake of
detector_reference.MUTATIONS would change the expected result of some case.

The kernel marches 16-lane strips of 56 output columns down segments of 32, 64 or 128 rows (detector_reference.seg_rows), so
the seams are at the widths 16 + 56 k and the heights 16 + 32 k.  It takes the cell size and the grid apart (cell_w, cell_h,
det_cols), the C ABI always hands it ceil-sized cells: at 137 x 89 no grid gives cells 56 or 57 wide or 31 .. 65 high that way,
so those cases (Case.ceil false) set the cell size themselves; their expected maxima are the oracle's per-pixel scores (its
maxima over a grid of one-pixel cells) reduced by detector_reference.reduce_cells, which test_detector_cases.py compares with
the oracle's own reduction on every ceil-sized case, cells of those sizes on other images included."""
import collections

import numpy as np

import detector_reference as DR

Case = collections.namedtuple("Case", "name kind w h rows cols cw ch floor seed")
Case.ceil = property(lambda c: (c.cw, c.ch) == DR.ceil_cells(c.w, c.h, c.rows, c.cols))

KINDS = ["checker8", "checker2", "checker1", "vstripes8", "hstripes8", "diagonal", "ramp", "flat", "random", "tile", "blocks", "half"]
ALL_TIE = {"checker8": 1280000, "checker2": 8323200}          # every valid pixel has this score
ZERO_SCORE = ["vstripes8", "hstripes8", "diagonal", "checker1", "flat"]
STRUCTURED = ["checker8", "checker2", "checker1", "vstripes8", "hstripes8", "diagonal", "ramp", "flat"]
TILE_W, TILE_H = 24, 20

_images = {}


def image(kind, w, h, seed=0):
    key = (kind, w, h, seed)
    if key not in _images:
        yy, xx = np.mgrid[0:h, 0:w]
        rng = np.random.default_rng([KINDS.index(kind), w, h, seed])
        if kind == "checker8":
            img = ((xx // 8 + yy // 8) % 2) * 200 + 20
        elif kind == "checker2":
            img = ((xx // 2 + yy // 2) % 2) * 255
        elif kind == "checker1":
            img = ((xx + yy) % 2) * 255
        elif kind == "vstripes8":
            img = ((xx // 8) % 2) * 200 + 20
        elif kind == "hstripes8":
            img = ((yy // 8) % 2) * 200 + 20
        elif kind == "diagonal":
            img = (((xx + yy) // 3) % 2) * 255
        elif kind == "ramp":
            img = (3 * xx + 2 * yy) % 256
        elif kind == "flat":
            img = np.full((h, w), 131)
        elif kind == "random":
            img = rng.integers(0, 256, (h, w))
        elif kind == "tile":
            t = np.random.default_rng(seed + 2420).integers(0, 256, (TILE_H, TILE_W))
            img = np.tile(t, (h // TILE_H + 1, w // TILE_W + 1))[:h, :w]
        elif kind == "blocks":
            base = rng.integers(0, 256, (h // 6 + 1, w // 6 + 1))
            img = (np.kron(base, np.ones((6, 6), np.int64))[:h, :w] + rng.integers(-9, 10, (h, w))).clip(0, 255)
        elif kind == "half":            # nothing to find left of the middle
            img = np.where(xx < w // 2, 131, rng.integers(0, 256, (h, w)))
        else:
            raise KeyError(kind)
        img = np.ascontiguousarray(img, dtype=np.uint8)
        img.setflags(write=False)
        _images[key] = img
    return _images[key]


def ceil_grid(name, kind, w, h, rows, cols, floor=0, seed=0):
    cw, ch = DR.ceil_cells(w, h, rows, cols)
    return Case(name, kind, w, h, rows, cols, cw, ch, floor, seed)


def cell_grid(name, kind, w, h, cw, ch, floor=0, seed=0):
    """The grid of cells cw x ch that covers the image."""
    return Case(name, kind, w, h, (h + ch - 1) // ch, (w + cw - 1) // cw, cw, ch, floor, seed)


def like16(name, kind, w, h, floor=0, seed=0):
    """Ceil-sized cells of about 16 x 16, as the default 47 x 30 grid gives at 752 x 480."""
    return ceil_grid(name, kind, w, h, (h + 15) // 16, (w + 15) // 16, floor, seed)


# ---- the geometry lists
WIDTHS = [17, 18, 19, 20] + [16 + 56 * k + d for k in (1, 2) for d in (-1, 0, 1, 2, 3, 4)]
HEIGHTS = [17] + [16 + 32 * k + d for k in (1, 2, 3) for d in (-1, 0, 1)]
TINY = [(17, 17), (17, 18), (18, 17), (20, 20)]
GW, GH = 137, 89                                          # three strips, three segments of 32 rows
CELL_WS = [1, 2, 3, 4, 5, 6, 7, 56, 57, GW]
CELL_HS = [1, 7, 8, 31, 32, 33, 65, GH]
GEOMETRY_KINDS = ["random", "tile", "checker8"]
LONG_W, LONG_H = 72, 4112                                 # one strip, 128 segments of 32 rows


def width_cases():
    return [like16("w%d" % w, "random", w, 40, seed=w) for w in WIDTHS]


def height_cases():
    return [like16("h%d" % h, "random", 72, h, seed=h) for h in HEIGHTS]


def tiny_cases():
    return [cell_grid("tiny%dx%d" % (w, h), "random", w, h, 4, 4, seed=w + h) for (w, h) in TINY]


def geometry_cases(kind):
    out = [cell_grid("%s_cw%d" % (kind, cw), kind, GW, GH, cw, 15) for cw in CELL_WS]
    out += [cell_grid("%s_ch%d" % (kind, ch), kind, GW, GH, 16, ch) for ch in CELL_HS]
    return out + [one_cell_case(kind)]


def one_cell_case(kind):
    return ceil_grid("%s_one_cell" % kind, kind, GW, GH, 1, 1)


def ceil_big_cell_cases():
    """Cells 56 and 57 wide, 31, 32, 33 and 65 high from the ceil rule itself, on the smallest images that give them."""
    out = [ceil_grid("ceil_cw%d" % (w // 3), "random", w, 40, 3, 3, seed=w) for w in (168, 171)]
    return out + [ceil_grid("ceil_ch%d" % ch, "random", 72, h, rows, 5, seed=h) for ch, h, rows in ((31, 93, 3), (32, 96, 3), (33, 99, 3), (65, 130, 2))]


def structured_cases():
    return [like16("structured_" + kind, kind, GW, GH) for kind in STRUCTURED]


def floor_cases():
    """The constant-score images with the floor at the score, one below and one above."""
    return [like16("%s_floor%+d" % (kind, d), kind, GW, GH, floor=ALL_TIE[kind] + d) for kind in ALL_TIE for d in (-1, 0, 1)]


def stale_case():
    return like16("stale_half", "half", GW, GH)


def long_cases():
    """The seven combinations the long-segment launches cycle through: three images, cells 103, 64 and 1 rows high, two floors
    (one at about the median of the random image's maxima, one a single step below the checkerboard's constant score)."""
    W, H = LONG_W, LONG_H
    return [ceil_grid("long_random_ch103", "random", W, H, 40, 1),
            ceil_grid("long_tile_ch103", "tile", W, H, 40, 11),
            ceil_grid("long_checker8_ch103", "checker8", W, H, 40, 18),
            ceil_grid("long_random_ch64_floor", "random", W, H, 65, 11, floor=1650000),
            ceil_grid("long_tile_ch64", "tile", W, H, 65, 1),
            ceil_grid("long_random_ch1", "random", W, H, H, 1),
            ceil_grid("long_checker8_ch103_floor", "checker8", W, H, 40, 1, floor=ALL_TIE["checker8"] - 1)]


MIXED_SHAPES = [(200, 130), (40, 130), (200, 30), (17, 17), (200, 17), (73, 49), (129, 81), (72, 48), (185, 113), (20, 129), (128, 47)]
MIXED_GRIDS = [(8, 12), (9, 3), (2, 25), (1, 1), (1, 40), (5, 7), (30, 47), (3, 4), (6, 1), (129, 20), (4, 9)]       # rows, cols


def mixed_cases():
    """Eleven streams of different sizes and grids for one launch cut for the largest (200 x 130): one narrower than a strip, one
    shorter than a segment, the smallest image, one as wide as the cut and 17 rows high, sizes at and beside the seams."""
    kinds = ["random", "blocks", "tile", "random", "random", "blocks", "random", "checker8", "random", "random", "blocks"]
    floors = {5: 500000, 8: 1900000}            # about the median of the stream's maxima: some cells lose theirs, others keep them
    return [ceil_grid("mixed%d_%dx%d" % (k, w, h), kinds[k], w, h, r, c, floor=floors.get(k, 0), seed=k)
            for k, ((w, h), (r, c)) in enumerate(zip(MIXED_SHAPES, MIXED_GRIDS))]


ABI_SHAPES = [(64, 64), (129, 81), (188, 120)]
ABI_GRIDS = [(7, 9), (30, 47), (3, 2)]                    # rows, cols


def abi_cases(push):
    """Nine streams of three sizes, each size with a grid of its own, for one push through the C ABI; push = 0, 1: the images differ."""
    kinds = ["random", "blocks", "tile"]
    return [ceil_grid("abi%d_push%d" % (k, push), kinds[(k + push) % 3], *ABI_SHAPES[k % 3], *ABI_GRIDS[k % 3], seed=10 * push + k) for k in range(9)]


def all_cases():
    out = width_cases() + height_cases() + tiny_cases() + ceil_big_cell_cases() + structured_cases() + floor_cases() + [stale_case()]
    for kind in GEOMETRY_KINDS:
        out += geometry_cases(kind)
    out += [one_cell_case(kind) for kind in ALL_TIE if kind not in GEOMETRY_KINDS]
    out += long_cases() + mixed_cases() + abi_cases(0) + abi_cases(1)
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return out


# ---- what the oracle says
_scores, _expected = {}, {}


def oracle_scores(oracle, case):
    """The oracle's score of every pixel: its maxima over a grid of one-pixel cells."""
    key = (case.kind, case.w, case.h, case.seed)
    if key not in _scores:
        s = oracle.cell_maxima(image(*key), case.h, case.w)["score"].astype(np.int64).reshape(case.h, case.w)
        s.setflags(write=False)
        _scores[key] = s
    return _scores[key]


def expected(oracle, case):
    """RESULT records of the case from the oracle: its own per-cell maxima above the floor where the cells are ceil-sized, its
    scores reduced over the case's cells otherwise.  Computed once, read-only."""
    if case not in _expected:
        if case.ceil:
            ref = oracle.cell_maxima(image(case.kind, case.w, case.h, case.seed), case.rows, case.cols)
            out = np.zeros(len(ref), DR.RESULT)
            out["has"] = ref["score"] > case.floor
            for k in ("score", "x", "y"):
                out[k] = np.where(out["has"], ref[k].astype(np.int64), 0)
        else:
            out = DR.reduce_cells(oracle_scores(oracle, case), case.rows, case.cols, case.cw, case.ch, case.floor)
        out.setflags(write=False)
        _expected[case] = out
    return _expected[case]


_restated_scores = {}


def restated(case, mutate=None):
    """RESULT records of the case from the numpy restatement (the score map of an image is computed once per way of scoring)."""
    key = (case.kind, case.w, case.h, case.seed, mutate if mutate in DR.SCORE_MUTATIONS else None)
    if key not in _restated_scores:
        _restated_scores[key] = DR.score_map(image(*key[:4]), key[4])
    return DR.reduce_cells(_restated_scores[key], case.rows, case.cols, case.cw, case.ch, case.floor, mutate)
