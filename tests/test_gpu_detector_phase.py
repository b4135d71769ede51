"""k_detect_cells forms the horizontal sums of one row difference per step (entering row minus leaving row) and scores a row
before the window moves on: the per-cell maxima must still be flushed at the bottom row of every cell, not one row early or
late.  Cells one row high (a flush after every step), eight rows high (the window's own height) and 32 rows high (a segment of
the march: the cell ends where the segment does), on a random image (every row's maximum differs) and on a flat one (nothing
anywhere: no stale key may survive from the push before)."""
import numpy as np
import pytest

from msckf_stereo_c_amd import capi
from msckf_stereo_c_amd.ctypes_types import default_ekf_cfg, default_fe_cfg

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("cell_h", [1, 8, 32])
def test_detector_cell_heights(gpu_ctx, oracle, cell_h):
    w, h = 128, 96
    det_rows, det_cols = h // cell_h, 16
    fe = default_fe_cfg()
    fe.det_rows, fe.det_cols = det_rows, det_cols
    rng = np.random.default_rng(cell_h)
    rnd = rng.integers(0, 256, (h, w), dtype=np.uint8)
    flat = np.full((h, w), 131, np.uint8)
    s = capi.Stream(gpu_ctx, oracle.euroc_calib(w, h), fe, default_ekf_cfg())
    for img in (rnd, flat, rnd):
        s.push_stereo(img, img)
        got, ref = s.cell_maxima(), oracle.cell_maxima(img, det_rows, det_cols)
        for k in ("score", "x", "y"):
            assert np.array_equal(got[k], ref[k]), k
    # (the random image is a real test: most of the cells that hold a scored pixel record a corner)
    assert (oracle.cell_maxima(rnd, det_rows, det_cols)["score"] > 0).sum() > (h - 16) // cell_h * (det_cols - 2) // 2
    s.close()
