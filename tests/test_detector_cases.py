"""The detector's case set (tests/detector_cases.py) and its numpy restatement (tests/detector_reference.py) on the CPU: the
restatement equals the oracle on every case, every planted mistake changes what some case expects, and the images do what they
were chosen for."""
import numpy as np
import pytest

import detector_cases as DC
import detector_reference as DR

CASES = DC.all_cases()


def _same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("has", "score", "x", "y"))


def test_restatement_equals_the_oracle(oracle):
    """Score, x and y of every cell of every case; on the cases that set their own cell size, also the score of every pixel."""
    for c in CASES:
        got, ref = DC.restated(c), DC.expected(oracle, c)
        assert len(got) == len(ref) == c.rows * c.cols
        assert _same(got, ref), c.name
        if not c.ceil:
            assert np.array_equal(DR.score_map(DC.image(c.kind, c.w, c.h, c.seed)), DC.oracle_scores(oracle, c)), c.name
    # cells of the sizes that 137 x 89 only has with a cell size of its own also come out of the ceil rule somewhere
    for sizes, pick in ((DC.CELL_WS, lambda c: c.cw), (DC.CELL_HS, lambda c: c.ch)):
        assert set(sizes) <= {pick(c) for c in CASES if c.ceil}


def test_the_launcher_rule():
    """What the long-segment launches rely on, and the 752 x 480 launches of DESIGN.md section 6."""
    assert [DR.seg_rows(n, DC.LONG_W, DC.LONG_H) for n in (7, 1024, 1025, 2048, 2049)] == [32, 32, 64, 64, 128]
    assert [DR.seg_rows(n, 752, 480) for n in (192, 624, 625, 1024, 1170, 1171)] == [32, 32, 64, 64, 64, 128]


def _mutant_changes(case, mutation):
    if mutation == "stale_wins":
        # keys of the generation before, with the largest score, in every cell: the launch must replace those of the cells it scores
        sent = DR.keys_of(DC.restated(case), case.cols, case.cw, case.ch, 2)
        before = np.full(len(sent), (1 << 56) | (0xFFFFFF << 32) | 0xFFFFFFFF, np.uint64)
        return not np.array_equal(DR.merge_keys(before, sent), DR.merge_keys(before, sent, mutation))
    return not _same(DC.restated(case), DC.restated(case, mutation))


@pytest.mark.parametrize("mutation", DR.MUTATIONS)
def test_the_set_sees_mutations(mutation):
    """Each planted mistake changes the expected result of at least one case (the long images stand for themselves: only the
    mistakes at the ends of segments are tried on them).  No image scores 2^23 or more, so masking the score to 23 bits is
    the one mistake nothing can show; the same mask one bit shorter has to be seen."""
    segs = mutation.startswith("drop_seg")
    cases = [c for c in CASES if segs or c.h < 1000]
    if mutation == "stale_wins":
        cases = [DC.stale_case()]
    caught = [c.name for c in cases if _mutant_changes(c, mutation)]
    print("%s: caught by %d cases: %s" % (mutation, len(caught), " ".join(caught)))
    if mutation == "mask23":
        assert DR.max_score() == DC.ALL_TIE["checker2"] < 1 << 23 and not caught
        return
    assert caught
    if segs:            # ... and by the long images the segments of 64 and 128 rows are launched on
        assert any(n.startswith("long_") for n in caught)
    if mutation == "mask22":
        assert any("checker2" in n for n in caught)
    if mutation in ("tie_last", "isqrt_square_low"):
        assert any("checker8" in n for n in caught)


def test_all_tie_images():
    """Every valid pixel of the two checkerboards has the same score, the discriminant of the period-8 one a perfect square
    everywhere; one cell over the image records its first valid pixel."""
    for kind, score in DC.ALL_TIE.items():
        img = DC.image(kind, DC.GW, DC.GH)
        s = DR.score_map(img)
        assert (s[DR.valid_mask(DC.GW, DC.GH)] == score).all(), kind
        one = DC.restated(DC.one_cell_case(kind))
        assert (one["score"][0], one["x"][0], one["y"][0]) == (score, 8, 8)
    a, b, c = DR.box_sums(DC.image("checker8", DC.GW, DC.GH))
    disc = ((a - c) ** 2 + 4 * b * b)[DR.valid_mask(DC.GW, DC.GH)]
    root = np.sqrt(disc.astype(np.float64)).astype(np.int64)
    assert (root * root == disc).all()


def test_zero_score_images():
    """Nothing is recorded on them, with a + c positive on the striped ones (only an exact square root gives the zero)."""
    for kind in DC.ZERO_SCORE:
        img = DC.image(kind, DC.GW, DC.GH)
        assert not DC.restated(DC.like16("z", kind, DC.GW, DC.GH))["has"].any(), kind
        a, _, c = DR.box_sums(img)
        if kind in ("vstripes8", "hstripes8", "diagonal"):
            assert ((a + c)[DR.valid_mask(DC.GW, DC.GH)] > 0).all(), kind
    # the floor decides with a strict >: at the score nothing, one below it every cell that has a valid pixel, its first one
    for c in DC.floor_cases():
        r = DC.restated(c)
        if c.floor >= DC.ALL_TIE[c.kind]:
            assert not r["has"].any(), c.name
        else:
            cells = np.arange(len(r))
            x0, y0 = np.maximum(cells % c.cols * c.cw, 8), np.maximum(cells // c.cols * c.ch, 8)
            assert r["has"].all() and np.array_equal(r["x"], x0) and np.array_equal(r["y"], y0), c.name


def test_repeated_tile_ties():
    """A cell whose valid pixels span two tiles in a direction holds its maximum at two pixels or more; in most of them the
    winner is not the cell's first valid pixel.  Most of the cells of the cases with such cells are of that kind."""
    seen = 0
    for c in CASES:
        if c.kind != "tile" or (c.cw < 2 * DC.TILE_W and c.ch < 2 * DC.TILE_H):
            continue
        s, r = DR.score_map(DC.image(c.kind, c.w, c.h, c.seed)), DC.restated(c)
        cells = np.flatnonzero(r["has"])
        wide = first = 0
        for k in cells:
            y0, x0 = k // c.cols * c.ch, k % c.cols * c.cw
            if min(x0 + c.cw, c.w - 8) - max(x0, 8) < 2 * DC.TILE_W and min(y0 + c.ch, c.h - 8) - max(y0, 8) < 2 * DC.TILE_H:
                continue
            wide += 1
            assert (s[y0:y0 + c.ch, x0:x0 + c.cw] == r["score"][k]).sum() >= 2, (c.name, k)
            first += int((r["x"][k], r["y"][k]) == (max(x0, 8), max(y0, 8)))
        assert 2 * wide >= len(cells) > 0 and 2 * first < wide, c.name
        seen += 1
    assert seen >= 4


def test_random_cases_are_alive():
    """Every random case records a corner in more than half of the cells that hold a valid pixel; the floors of the long and
    the mixed cases remove some maxima and leave others."""
    for c in CASES:
        if c.kind not in ("random", "blocks"):
            continue
        r = DC.restated(c)
        cells = np.arange(len(r))
        x0, y0 = cells % c.cols * c.cw, cells // c.cols * c.ch
        holds = (x0 < c.w - 8) & (x0 + c.cw > 8) & (y0 < c.h - 8) & (y0 + c.ch > 8)
        assert not r["has"][~holds].any()
        if c.floor:
            free = DC.restated(c._replace(floor=0))
            assert 0 < r["has"].sum() < free["has"].sum(), c.name
        else:
            assert 2 * r["has"].sum() > holds.sum(), c.name
