"""GPU parity tests of the hand-written HIP kernels against the CPU oracle, through the C-ABI.

Bar (BASELINE.json north_star): integer / pixel / id work bit-exact; EKF doubles within 1e-9
relative at the kernel level (the end-to-end pose bar is 1e-4 m / 1e-4 rad).
"""
import numpy as np
import pytest

from msckf_stereo_c_amd import capi
from msckf_stereo_c_amd.ctypes_types import default_ekf_cfg, default_fe_cfg

import ekf_problems

pytestmark = pytest.mark.gpu


def _stream(gpu_ctx, oracle, w, h, **kw):
    calib = oracle.euroc_calib(w, h)
    return capi.Stream(gpu_ctx, calib, default_fe_cfg(), default_ekf_cfg(**kw)), calib


@pytest.mark.parametrize("w,h", [(752, 480), (376, 240), (333, 251), (1280, 720), (64, 64), (65, 67), (129, 71), (255, 130), (257, 193), (1001, 99), (122, 509)])
def test_pyramid_bit_exact(gpu_ctx, oracle, w, h):
    """Levels 1 .. 3 from the one-launch kernel (k_pyr_down3: a register / DPP row march, a 16-lane strip owns 12 level-3
    columns and marches down a segment of level-3 rows, borders reflected per level) equal three separate pyr_down passes of
    the oracle bit for bit: the benchmark shapes, odd sizes at every level, sizes one pixel either side of 128 x 64 pixels of
    level 0, the smallest images a stream accepts, long thin images.  The seams of the march itself (strips of 96 level-0
    columns, segments) are the subject of tests/test_gpu_pyramid_march.py."""
    rng = np.random.default_rng(w * 1000 + h)
    a = rng.integers(0, 256, (h, w), dtype=np.uint8)
    b = rng.integers(0, 256, (h, w), dtype=np.uint8)
    s, _ = _stream(gpu_ctx, oracle, w, h)
    s.push_stereo(a, b)
    for role, img in ((1, a), (2, b)):
        ref = oracle.build_pyramid(img)
        for lvl in range(4):
            got = s.get_level(role, lvl)
            assert got.shape == ref[lvl].shape
            assert np.array_equal(got, ref[lvl]), (role, lvl)
    s.close()


@pytest.mark.parametrize("w,h,seed", [(376, 240, 0x5EED0000), (752, 480, 0x5EED0007), (188, 120, 11)])
def test_device_renderer_equals_host(gpu_ctx, oracle, w, h, seed):
    """The input generator on the device (csrc/synth/synth_render.hip, what bench.py renders its sequences with) produces the
    bytes of the host generator (synth.h, what every parity test and the CPU oracle's legs use): static prefix, moving frames,
    both cameras, the wrap of the looping trajectory."""
    from msckf_stereo_c_amd import synth_device
    syn = oracle.Synth(seed=seed, width=w, height=h, n_static=3, n_loop=6)
    dev = synth_device.render_frames_to_host(syn, list(range(9)))
    for k in range(9):
        a, b = syn.render(k)
        assert np.array_equal(dev[0, k], a), (k, 0, int((dev[0, k] != a).sum()))
        assert np.array_equal(dev[1, k], b), (k, 1, int((dev[1, k] != b).sum()))


def test_pitched_host_images_are_repacked(gpu_ctx, oracle):
    """mskf_fe_push_stereo with pitch > width (padded rows, cv::Mat::step): the padding never reaches the pyramid."""
    w, h, pitch = 376, 240, 384
    rng = np.random.default_rng(7)
    a = rng.integers(0, 256, (h, pitch), dtype=np.uint8)
    b = rng.integers(0, 256, (h, pitch), dtype=np.uint8)
    s, _ = _stream(gpu_ctx, oracle, w, h)
    s.push_stereo(a, b, pitch=pitch)
    for role, img in ((1, a[:, :w]), (2, b[:, :w])):
        ref = oracle.build_pyramid(np.ascontiguousarray(img))
        for lvl in range(4):
            assert np.array_equal(s.get_level(role, lvl), ref[lvl]), (role, lvl)
    s.close()


@pytest.mark.parametrize("w,h,seed", [(752, 480, 1), (376, 240, 2), (1280, 720, 3)])
def test_detector_bit_exact(gpu_ctx, oracle, w, h, seed):
    syn = oracle.Synth(seed=seed, width=w, height=h)
    a, b = syn.render(3)
    s, _ = _stream(gpu_ctx, oracle, w, h)
    s.push_stereo(a, b)
    got = s.cell_maxima()
    ref = oracle.cell_maxima(a)
    assert np.array_equal(got["score"], ref["score"])
    assert np.array_equal(got["x"], ref["x"]) and np.array_equal(got["y"], ref["y"])
    assert (ref["score"] > 2560).sum() > 100   # the scene is textured enough to be a real test
    s.close()


def test_detector_flat_and_ties(gpu_ctx, oracle):
    w, h = 376, 240
    flat = np.full((h, w), 77, np.uint8)
    # a periodic pattern produces exact score ties inside a cell: the first in row-major order must win
    yy, xx = np.mgrid[0:h, 0:w]
    tie = (((xx // 8) + (yy // 8)) % 2 * 200 + 20).astype(np.uint8)
    s, _ = _stream(gpu_ctx, oracle, w, h)
    for img in (flat, tie):
        s.push_stereo(img, img)
        got, ref = s.cell_maxima(), oracle.cell_maxima(img)
        for k in ("score", "x", "y"):
            assert np.array_equal(got[k], ref[k]), k
    s.close()


@pytest.mark.parametrize("floor", [1, 10 * 256, 40 * 256, 300 * 256])
def test_detector_floor_is_exact(gpu_ctx, oracle, floor):
    """mskf_fe_set_detect_floor: only scores ABOVE the floor are recorded, decided before the integer square root
    (disc < (a + d - floor)^2).  The recorded maxima must be exactly the oracle's maxima above the floor (score, position,
    tie-break), everything else reads as "no corner", and candidates cannot be asked for below the floor."""
    for w, h, seed in ((752, 480, 11), (376, 240, 12)):
        syn = oracle.Synth(seed=seed, width=w, height=h)
        a, b = syn.render(5)
        s, _ = _stream(gpu_ctx, oracle, w, h)
        s.set_detect_floor(floor)
        s.push_stereo(a, b)
        got, ref = s.cell_maxima(), oracle.cell_maxima(a)
        keep = ref["score"] > floor
        assert np.array_equal(got["score"], np.where(keep, ref["score"], 0))
        assert np.array_equal(got["x"][keep], ref["x"][keep]) and np.array_equal(got["y"][keep], ref["y"][keep])
        cand = s.cell_candidates(floor)
        assert len(cand) == keep.sum() and np.array_equal(cand["score"], ref["score"][keep])
        if floor > 1:
            with pytest.raises(Exception):
                s.cell_candidates(floor - 1)
        # back to "every positive score" with the next push
        s.set_detect_floor(0)
        s.push_stereo(a, b)
        assert np.array_equal(s.cell_maxima()["score"], ref["score"])
        s.close()


def test_cell_candidates_are_the_maxima_above_threshold(gpu_ctx, oracle):
    """mskf_fe_get_cell_candidates == the records of mskf_fe_get_cell_maxima with score > min_score, in cell order."""
    syn = oracle.Synth(seed=5, width=752, height=480)
    a, b = syn.render(7)
    s, _ = _stream(gpu_ctx, oracle, 752, 480)
    s.push_stereo(a, b)
    full = s.cell_maxima()
    for thr in (0, 10 * 256, 40 * 256, 10 ** 9):
        cand = s.cell_candidates(thr)
        want = full[full["score"] > thr]
        assert len(cand) == len(want)
        for f in ("x", "y", "score", "cell"):
            assert np.array_equal(cand[f], want[f]), f
    assert len(s.cell_candidates(10 * 256)) > 100
    s.close()


@pytest.mark.parametrize("w,h,seed", [(752, 480, 11), (376, 240, 12)])
def test_lk_temporal_and_stereo_bit_exact(gpu_ctx, oracle, w, h, seed):
    syn = oracle.Synth(seed=seed, width=w, height=h)
    a0, b0 = syn.render(40)
    a1, b1 = syn.render(41)
    s, calib = _stream(gpu_ctx, oracle, w, h)
    fe = default_fe_cfg()
    s.push_stereo(a0, b0)
    pts, _ = oracle.detect(a0)
    # add hard cases: border points, out-of-image points, a flat-region-free random set
    rng = np.random.default_rng(seed)
    extra = np.stack([rng.uniform(-20, w + 20, 64), rng.uniform(-20, h + 20, 64)], 1).astype(np.float32)
    pts = np.concatenate([pts, extra, np.array([[0, 0], [w - 1, h - 1], [3.5, 2.25], [w - 2.5, 7.75]], np.float32)])
    # sub-pixel offsets whose 14-bit fractions multiply to 8192: the fourth bilinear weight is -1 there
    # (16384 - w00 - w01 - w10 with all three rounded up), which the packed 16-bit dot products must reproduce
    det = pts[:40].copy()
    for k, (fa, fb) in enumerate([(64, 128), (2, 4096), (8192, 1), (128, 64), (1024, 8), (16, 512)]):
        det[k::6] = np.floor(det[k::6]) + np.array([fa / 16384.0, fb / 16384.0], np.float32)
    pts = np.concatenate([pts, det]).astype(np.float32)
    s.swap()
    s.push_stereo(a1, b1)
    # --- temporal + stereo (trackFeatures path)
    got = s.track(pts, do_temporal=True)
    ref_b, ref_st = oracle.lk_track(a0, a1, pts, pts.copy())
    ok = ref_st.astype(bool)
    ok &= ~((ref_b[:, 1] < 0) | (ref_b[:, 1] > h - 1) | (ref_b[:, 0] < 0) | (ref_b[:, 0] > w - 1))
    assert np.array_equal((got["status"] & 1).astype(bool), ok)
    assert np.array_equal(got["out0"][ok], ref_b[ok])
    assert ok.sum() > 50
    # stereo stage of the tracked points
    tracked = ref_b[ok]
    ref_c1, ref_in = oracle.stereo_match(calib, fe, a1, b1, tracked)
    assert np.array_equal(((got["status"][ok] >> 1) & 1), ref_in)
    assert np.array_equal(got["out1"][ok], ref_c1)
    assert ref_in.sum() > 30
    # undistorted coordinates used by publish()
    K0, D0 = np.array(calib.cam0_intrinsics), np.array(calib.cam0_distortion)
    K1, D1 = np.array(calib.cam1_intrinsics), np.array(calib.cam1_distortion)
    assert np.array_equal(got["und0"][ok], oracle.undistort(K0, D0, tracked))
    assert np.array_equal(got["und1"][ok], oracle.undistort(K1, D1, ref_c1))
    # --- stereo only (initializeFirstFrame / addNewFeatures path)
    cand, _ = oracle.detect(a1)
    got2 = s.track(cand, do_temporal=False)
    ref_c1, ref_in = oracle.stereo_match(calib, fe, a1, b1, cand)
    assert np.array_equal((got2["status"] >> 1) & 1, ref_in)
    assert np.array_equal(got2["out1"], ref_c1)
    assert np.array_equal(got2["out0"], cand)
    s.close()


def test_ekf_propagate_augment_remove(gpu_ctx, oracle):
    s, calib = _stream(gpu_ctx, oracle, 376, 240, max_cam_state_size=8)
    rng = np.random.default_rng(5)
    A = rng.normal(size=(21, 21))
    P = A @ A.T * 1e-3
    P = (P + P.T) / 2
    s.ekf_reset(P)
    Pref = P.copy()
    for rnd in range(5):
        # augment
        J = rng.normal(size=(6, 21))
        d = Pref.shape[0]
        s.ekf_augment(J)
        Pn = np.zeros((d + 6, d + 6))
        Pn[:d, :d] = Pref
        Pn[d:, :d] = J @ Pref[:21, :d]
        Pn[:d, d:] = Pn[d:, :d].T
        Pn[d:, d:] = J @ Pref[:21, :21] @ J.T
        Pref = (Pn + Pn.T) / 2
        # propagate 10 steps
        Phi = np.eye(21) + rng.normal(size=(10, 21, 21)) * 1e-2
        Q = np.stack([(lambda B: B @ B.T * 1e-6)(rng.normal(size=(21, 21))) for _ in range(10)])
        s.ekf_propagate(Phi, Q)
        for k in range(10):
            d = Pref.shape[0]
            Pn = Pref.copy()
            Pn[:21, :21] = Phi[k] @ Pref[:21, :21] @ Phi[k].T + Q[k]
            Pn[:21, 21:] = Phi[k] @ Pref[:21, 21:]
            Pn[21:, :21] = Pref[21:, :21] @ Phi[k].T
            Pref = (Pn + Pn.T) / 2
        got = s.ekf_get_cov()
        assert got.shape == Pref.shape
        assert np.allclose(got, Pref, rtol=1e-12, atol=1e-15)
        assert np.array_equal(got, got.T)
    # remove clones 1 then 0
    for idx in (1, 0):
        s.ekf_remove_clone(idx)
        keep = [i for i in range(Pref.shape[0]) if not (21 + 6 * idx <= i < 27 + 6 * idx)]
        Pref = Pref[np.ix_(keep, keep)]
        got = s.ekf_get_cov()
        assert np.allclose(got, Pref, rtol=1e-12, atol=1e-15)
    s.close()


@pytest.mark.parametrize("n_clones,n_feat,seed,dof_offset", [(6, 5, 1, -1), (20, 30, 2, -1), (30, 60, 3, -1), (12, 20, 4, 0)])
def test_ekf_update_matches_oracle(gpu_ctx, oracle, n_clones, n_feat, seed, dof_offset):
    """The whole update against the oracle in the default configuration.  Since compression_mode 3 became the default of
    default_ekf_cfg() this is the Householder route (k_ekf_tsqr, then T, S, the factorisation of S, the solve and the
    downdate), not Gram + regularised Cholesky: the bars below were set for the Gram route and still carry its lambda prior.
    The Gram route, the fallback TSQR and the kernels' size limits are checked in value by tests/test_gpu_update_routes.py."""
    s, calib = _stream(gpu_ctx, oracle, 376, 240, max_cam_state_size=max(n_clones, 4))
    cfg = default_ekf_cfg(max_cam_state_size=max(n_clones, 4))
    pr = ekf_problems.make_problem(calib, seed=seed, n_clones=n_clones, n_feat=n_feat)
    ref = oracle.ekf_update_problem(calib, cfg, pr["gravity"], pr["clones"], pr["P"], pr["positions"], pr["obs_start"],
                                    pr["obs_clone"], pr["obs_z"], dof_offset)
    s.ekf_set_cov(pr["P"])
    got = s.ekf_update(pr["gravity"], pr["clones"], pr["positions"], pr["obs_start"], pr["obs_clone"], pr["obs_z"],
                       dof_offset, apply_row_cap=(dof_offset < 0))
    ev = ref["gamma"] >= 0          # the oracle stops evaluating features once the 1500-row cap is hit (Q13)
    assert np.allclose(got["gamma"][ev], ref["gamma"][ev], rtol=1e-7)
    assert np.array_equal((got["status"] >> 1) & 1, ref["passed"])
    assert got["rows"] == ref["rows"]
    assert ref["passed"].sum() >= 1
    scale = np.abs(ref["delta_x"]).max()
    assert np.allclose(got["delta_x"], ref["delta_x"], rtol=1e-6, atol=1e-9 * max(scale, 1e-3))
    Pg = s.ekf_get_cov()
    assert np.allclose(Pg, ref["P"], rtol=1e-7, atol=1e-8 * np.abs(ref["P"]).max())   # (wide enough for the Gram route's lambda-prior bias, ~1e-10)
    assert np.array_equal(Pg, Pg.T)
    s.close()


@pytest.mark.parametrize("n_clones,n_feat,pair,seed", [(30, 400, (3, 4), 31), (12, 70, (0, 1), 32), (20, 5, (17, 18), 33)])
def test_ekf_pruning_update_pair_path(gpu_ctx, oracle, n_clones, n_feat, pair, seed):
    """The pruning update's shape (msckf_vio.cpp:1073-1153): hundreds of features, each observed by exactly the two
    clones being removed, dof = 2, no row cap.  On the device that is the thread-per-feature kernel k_ekf_pair_blocks
    and the fused k_ekf_small_update (12 active columns); gates, gains and covariance against the oracle's generic
    featureJacobian / measurementUpdate."""
    s, calib = _stream(gpu_ctx, oracle, 376, 240, max_cam_state_size=n_clones)
    cfg = default_ekf_cfg(max_cam_state_size=n_clones)
    pr = ekf_problems.make_problem(calib, seed=seed, n_clones=n_clones, n_feat=n_feat, pair=pair, noise=0.004)
    ref = oracle.ekf_update_problem(calib, cfg, pr["gravity"], pr["clones"], pr["P"], pr["positions"], pr["obs_start"],
                                    pr["obs_clone"], pr["obs_z"], 0)
    s.ekf_set_cov(pr["P"])
    got = s.ekf_update(pr["gravity"], pr["clones"], pr["positions"], pr["obs_start"], pr["obs_clone"], pr["obs_z"], 0, False)
    assert np.allclose(got["gamma"], ref["gamma"], rtol=1e-7)
    assert np.array_equal((got["status"] >> 1) & 1, ref["passed"])
    assert 0 < ref["passed"].sum() and got["rows"] == ref["rows"] == 5 * ref["passed"].sum()
    scale = np.abs(ref["delta_x"]).max()
    assert np.allclose(got["delta_x"], ref["delta_x"], rtol=1e-6, atol=1e-9 * max(scale, 1e-3))
    Pg = s.ekf_get_cov()
    assert np.abs(Pg - ref["P"]).max() / np.abs(ref["P"]).max() < 1e-8
    assert np.array_equal(Pg, Pg.T)
    # the same through triangulation on the device (k_ekf_triangulate): positions from the two stereo views only
    s.ekf_set_cov(pr["P"])
    pos_ref, valid_ref = oracle.triangulate(calib, pr["clones"], pr["obs_start"], pr["obs_clone"], pr["obs_z"])
    got2 = s.ekf_update(pr["gravity"], pr["clones"], None, pr["obs_start"], pr["obs_clone"], pr["obs_z"], 0, False,
                        needs_init=np.ones(n_feat, np.int32))
    assert np.array_equal(got2["status"] & 1, valid_ref)
    v = valid_ref.astype(bool)
    assert np.allclose(got2["positions"][v], pos_ref[v], rtol=1e-6, atol=1e-8)
    s.close()


def test_triangulation_matches_oracle(gpu_ctx, oracle):
    n_clones = 12
    s, calib = _stream(gpu_ctx, oracle, 376, 240, max_cam_state_size=n_clones)
    pr = ekf_problems.make_problem(calib, seed=9, n_clones=n_clones, n_feat=25, noise=0.001)
    pos_ref, valid_ref = oracle.triangulate(calib, pr["clones"], pr["obs_start"], pr["obs_clone"], pr["obs_z"])
    s.ekf_set_cov(pr["P"])
    got = s.ekf_update(pr["gravity"], pr["clones"], None, pr["obs_start"], pr["obs_clone"], pr["obs_z"], -1, True,
                       needs_init=np.ones(25, np.int32))
    assert np.array_equal(got["status"] & 1, valid_ref)
    v = valid_ref.astype(bool)
    assert v.sum() >= 20
    assert np.allclose(got["positions"][v], pos_ref[v], rtol=1e-6, atol=1e-8)
    s.close()


# ------------------------------------------------------------------ large-configuration code paths
def test_detector_large_cells(gpu_ctx, oracle):
    """Cells larger than a 32-row segment of the detector's march and not a multiple of a lane's four columns (4K-like geometry:
    2000/47 = 43, 1100/30 = 37 px): cell rows cross the segment ends, where two segments feed a cell through atomicMax.  Cells
    wider than a strip and higher than several segments are in tests/test_gpu_detector_edges.py."""
    w, h = 2000, 1100
    rng = np.random.default_rng(4)
    base = rng.integers(0, 256, (h // 8 + 1, w // 8 + 1), dtype=np.uint8)
    img = np.kron(base, np.ones((8, 8), np.uint8))[:h, :w].copy()
    img = (img.astype(np.int32) + rng.integers(-6, 7, img.shape)).clip(0, 255).astype(np.uint8)
    s, _ = _stream(gpu_ctx, oracle, w, h)
    s.push_stereo(img, img)
    got, ref = s.cell_maxima(), oracle.cell_maxima(img)
    for k in ("score", "x", "y"):
        assert np.array_equal(got[k], ref[k]), k
    for lvl in range(4):
        assert np.array_equal(s.get_level(1, lvl), oracle.build_pyramid(img)[lvl])
    s.close()


@pytest.mark.parametrize("w,h", [(128, 96), (70, 64), (190, 130), (750, 478)])
def test_detector_small_and_odd_geometries(gpu_ctx, oracle, w, h):
    """Detector cells narrower than four pixels (width < 188 with the 47 x 30 grid: a lane's four columns touch up to three
    cells), cells that are not multiples of four, and image widths that are not multiples of four (the strip's last loads are
    clamped and unaligned)."""
    rng = np.random.default_rng(w * 1000 + h)
    base = rng.integers(0, 256, (h // 6 + 1, w // 6 + 1), dtype=np.uint8)
    img = np.kron(base, np.ones((6, 6), np.uint8))[:h, :w].copy()
    img = (img.astype(np.int32) + rng.integers(-9, 10, img.shape)).clip(0, 255).astype(np.uint8)
    s, _ = _stream(gpu_ctx, oracle, w, h)
    s.push_stereo(img, img)
    got, ref = s.cell_maxima(), oracle.cell_maxima(img)
    for k in ("score", "x", "y"):
        assert np.array_equal(got[k], ref[k]), k
    assert (ref["score"] > 0).sum() > 20
    for lvl in range(4):
        assert np.array_equal(s.get_level(1, lvl), oracle.build_pyramid(img)[lvl])
    s.close()


@pytest.mark.parametrize("n_clones,n_feat", [(29, 4), (13, 4), (24, 4), (30, 4), (10, 2), (19, 3)])
def test_ekf_update_ill_conditioned(gpu_ctx, oracle, n_clones, n_feat):
    """Few features over many clones: the stacked Jacobian is rank deficient beyond the gauge and cond(H) ~ 1e6-1e7.
    An unpivoted semidefinite Cholesky of H^T H loses up to 7e-5 here (tools/dev/update_truth.py), which is why the Gram route
    factors G + lambda I.  Since compression_mode 3 became the default of default_ekf_cfg() these stacks do NOT reach that
    factorisation any more: they run k_ekf_tsqr (rows > active columns) or the uncompressed route, Householder against the
    oracle's Householder, at the 1e-9 level asserted here.  The regularised factorisation on such stacks is checked in value in
    compression modes 0 and 1 by test_ekf_compression_condition_sweep and tests/test_gpu_update_routes.py."""
    s, calib = _stream(gpu_ctx, oracle, 376, 240, max_cam_state_size=max(n_clones, 4))
    cfg = default_ekf_cfg(max_cam_state_size=max(n_clones, 4))
    pr = ekf_problems.make_problem(calib, seed=100 + n_clones, n_clones=n_clones, n_feat=n_feat, min_obs=3)
    ref = oracle.ekf_update_problem(calib, cfg, pr["gravity"], pr["clones"], pr["P"], pr["positions"], pr["obs_start"],
                                    pr["obs_clone"], pr["obs_z"], -1)
    s.ekf_set_cov(pr["P"])
    got = s.ekf_update(pr["gravity"], pr["clones"], pr["positions"], pr["obs_start"], pr["obs_clone"], pr["obs_z"], -1, True)
    assert got["rows"] == ref["rows"] > 0
    Pg = s.ekf_get_cov()
    assert np.abs(Pg - ref["P"]).max() / np.abs(ref["P"]).max() < 2e-9
    assert np.abs(got["delta_x"] - ref["delta_x"]).max() / np.abs(ref["delta_x"]).max() < 2e-8
    s.close()


def _update_vs_oracle(gpu_ctx, oracle, n_clones, n_feat, seed, mode, dof_offset=-1, cap=True, **kw):
    calib = oracle.euroc_calib(376, 240)
    cfg = default_ekf_cfg(max_cam_state_size=max(n_clones, 4), compression_mode=mode)
    s = capi.Stream(gpu_ctx, calib, default_fe_cfg(), cfg)
    pr = ekf_problems.make_problem(calib, seed=seed, n_clones=n_clones, n_feat=n_feat, **kw)
    ref = oracle.ekf_update_problem(calib, cfg, pr["gravity"], pr["clones"], pr["P"], pr["positions"], pr["obs_start"],
                                    pr["obs_clone"], pr["obs_z"], dof_offset)
    s.ekf_set_cov(pr["P"])
    got = s.ekf_update(pr["gravity"], pr["clones"], pr["positions"], pr["obs_start"], pr["obs_clone"], pr["obs_z"], dof_offset, cap)
    Pg = s.ekf_get_cov()
    s.close()
    st = (got["status"] >> 1) & 1
    used = sorted(set(int(c) for j in range(n_feat) if st[j] for c in pr["obs_clone"][pr["obs_start"][j]:pr["obs_start"][j + 1]]))
    return dict(got=got, ref=ref, errP=np.abs(Pg - ref["P"]).max() / np.abs(ref["P"]).max(),
                errdx=np.abs(got["delta_x"] - ref["delta_x"]).max() / max(np.abs(ref["delta_x"]).max(), 1e-300),
                na=6 * len(used), sym=np.array_equal(Pg, Pg.T))


@pytest.mark.parametrize("n_clones,n_feat,seed,kw", [
    (6, 5, 1, {}), (20, 30, 2, {}), (30, 60, 3, {}),                                   # full-rank stacks, the 1500-row cap
    (29, 4, 129, dict(min_obs=3)), (13, 4, 113, dict(min_obs=3)), (10, 2, 110, dict(min_obs=3)),   # few features over many clones
    (13, 2, 1301, dict(min_obs=3)), (24, 2, 2402, dict(min_obs=3)),                    # fewer rows than active columns
    (50, 40, 21, dict(min_obs=20)), (64, 30, 23, dict(min_obs=20)),                    # R does not fit LDS: kept in the W buffer
    (30, 400, 31, dict(pair=(3, 4), noise=0.004)), (12, 2, 5, dict(pair=(0, 1))),      # pruning shape: inside k_ekf_small_update
])
def test_ekf_update_householder_tsqr(gpu_ctx, oracle, n_clones, n_feat, seed, kw):
    """compression_mode = 2: the QR compression of msckf_vio.cpp:795-817 as Householder row-block TSQR (k_ekf_qr /
    the TSQR branch of k_ekf_small_update) instead of Gram + Cholesky.  The oracle compresses with Householder QR too, so
    the two agree to rounding: 1e-9 is the bar, ~1e-15 is what comes out."""
    pair = "pair" in kw
    r = _update_vs_oracle(gpu_ctx, oracle, n_clones, n_feat, seed, 2, 0 if pair else -1, not pair, **kw)
    assert r["got"]["used_qr"] == 1
    assert r["got"]["rows"] == r["ref"]["rows"] > 0
    assert r["errP"] < 1e-9 and r["errdx"] < 1e-9 and r["sym"]
    assert r["errP"] < 1e-12                                   # (what Householder against Householder actually gives)


def test_ekf_update_rows_not_more_than_columns_skips_gram(gpu_ctx, oracle):
    """The reference's m <= d case (msckf_vio.cpp:818-821: no compression when the stack has no more rows than
    columns): in auto mode the Gram pass and its factorisation are skipped (H^T H would be singular by construction) and
    the stacked rows are the measurement as they are (S is rows x rows); with more rows than columns the default Gram
    path runs."""
    few = _update_vs_oracle(gpu_ctx, oracle, 13, 2, 1301, 0, min_obs=3)
    assert few["got"]["rows"] <= few["na"] and few["got"]["used_qr"] == 2        # 2 = used uncompressed
    assert few["errP"] < 1e-12 and few["errdx"] < 1e-9
    for n_clones, n_feat, seed in ((24, 2, 2402), (8, 2, 801), (30, 3, 3003)):
        r = _update_vs_oracle(gpu_ctx, oracle, n_clones, n_feat, seed, 0, min_obs=3)
        if r["got"]["rows"] <= r["na"]:
            assert r["got"]["used_qr"] == 2 and r["errP"] < 1e-12, (n_clones, n_feat, r["errP"])
    many = _update_vs_oracle(gpu_ctx, oracle, 13, 8, 1301, 0, min_obs=3)
    assert many["got"]["rows"] > many["na"] and many["got"]["used_qr"] == 0
    assert many["errP"] < 2e-9


def test_ekf_update_reference_rule(gpu_ctx, oracle):
    """compression_mode = 3 (the default of the host mirror and of bench.py): msckf_vio.cpp:795-821 as written - Householder QR
    when the stack has more rows than (active) columns, the stacked rows themselves otherwise.  Both branches against the
    oracle, which does the same: rounding level."""
    many = _update_vs_oracle(gpu_ctx, oracle, 13, 8, 1301, 3, min_obs=3)
    assert many["got"]["rows"] > many["na"] and many["got"]["used_qr"] == 1           # 1 = Householder
    assert many["errP"] < 1e-12 and many["errdx"] < 1e-9
    few = _update_vs_oracle(gpu_ctx, oracle, 13, 2, 1301, 3, min_obs=3)
    assert few["got"]["rows"] <= few["na"] and few["got"]["used_qr"] == 2             # 2 = uncompressed
    assert few["errP"] < 1e-12 and few["errdx"] < 1e-9
    big = _update_vs_oracle(gpu_ctx, oracle, 30, 60, 3, 3)                            # the 1500-row cap, R beside a 48-row block in LDS
    assert big["got"]["used_qr"] == 1 and big["errP"] < 1e-12
    prune = _update_vs_oracle(gpu_ctx, oracle, 30, 400, 31, 3, 0, False, pair=(3, 4), noise=0.004)    # pruning shape: 128-row blocks in the fused update
    assert prune["got"]["used_qr"] == 1 and prune["errP"] < 1e-12


def test_ekf_compression_condition_sweep(gpu_ctx, oracle):
    """Gram + regularised Cholesky squares cond(H) and adds the prior lambda I; how far can the stack be pushed before
    that shows?  The generator is driven towards ill conditioning (camera motion between clones shrunk to 1e-4, cond(H)
    beyond 1e9) and towards large Jacobian entries (features at a few centimetres).  Findings pinned here:
      * Householder TSQR stays at rounding level against the oracle's Householder QR everywhere;
      * the Gram path's error does NOT grow with cond(H): the update is regularised by P, the loss is the lambda prior,
        lambda max(P_aa) / sigma^2, and it grows with the SIZE of H (close features), as the device-side bound predicts;
      * auto mode switches to TSQR where the device-side bound predicts more than 1e-6 (QR_BIAS_LIMIT): it is on TSQR
        wherever the Gram path would exceed 1e-5 and stays below 1e-6 everywhere."""
    rows = []
    for baseline_scale, depth_scale in [(1.0, 1.0), (1e-1, 1.0), (1e-2, 1.0), (1e-3, 1.0), (1e-4, 1.0),
                                        (1.0, 0.3), (1.0, 0.1), (1.0, 0.03), (1.0, 0.01), (1.0, 0.004), (1e-2, 0.03)]:
        kw = dict(min_obs=3, baseline_scale=baseline_scale, depth_scale=depth_scale, noise=0.002)
        gram = _update_vs_oracle(gpu_ctx, oracle, 20, 12, 77, 1, **kw)
        tsqr = _update_vs_oracle(gpu_ctx, oracle, 20, 12, 77, 2, **kw)
        auto = _update_vs_oracle(gpu_ctx, oracle, 20, 12, 77, 0, **kw)
        rows.append((baseline_scale, depth_scale, gram["errP"], tsqr["errP"], auto["errP"], auto["got"]["used_qr"], gram["got"]["rows"]))
        print("baseline x%-6g depth x%-5g rows %4d  |dP|/|P|: gram %.2e  tsqr %.2e  auto %.2e (tsqr used: %d)" % (
            baseline_scale, depth_scale, gram["got"]["rows"], gram["errP"], tsqr["errP"], auto["errP"], auto["got"]["used_qr"]))
    for b, dsc, eg, et, ea, used, nrows in rows:
        if nrows == 0:
            continue
        assert et < 1e-9, (b, dsc, et)
        assert ea < 1e-6, (b, dsc, ea)
        if eg > 1e-5:
            assert used == 1, (b, dsc, eg)
    assert max(r[2] for r in rows if r[1] == 1.0 and r[6] > 0) < 1e-8        # conditioning alone never hurts the Gram path


@pytest.mark.parametrize("n_clones,n_feat,seed", [(50, 40, 21), (60, 30, 22), (64, 30, 23)])
def test_ekf_update_many_clones(gpu_ctx, oracle, n_clones, n_feat, seed):
    """d = 321 / 381 / 405 (the largest window mskf_stream_create accepts): gating matrix outside LDS, > 1500 stacked rows
    (cap), the triangular solve's strip at its LDS limit.  Since compression_mode 3 became the default of default_ekf_cfg() the
    stack is compressed by k_ekf_tsqr<16,4,2> with R in the W buffer; the global-memory Cholesky k_ekf_chol runs here on the
    innovation covariance only (which == 1).  Its Gram variant (which == 0) at these windows is checked by
    tests/test_gpu_update_routes.py (31, 32, 34, 35 and 64 clones in mode 1)."""
    s, calib = _stream(gpu_ctx, oracle, 376, 240, max_cam_state_size=n_clones)
    cfg = default_ekf_cfg(max_cam_state_size=n_clones)
    pr = ekf_problems.make_problem(calib, seed=seed, n_clones=n_clones, n_feat=n_feat, min_obs=20)
    ref = oracle.ekf_update_problem(calib, cfg, pr["gravity"], pr["clones"], pr["P"], pr["positions"], pr["obs_start"],
                                    pr["obs_clone"], pr["obs_z"], -1)
    s.ekf_set_cov(pr["P"])
    got = s.ekf_update(pr["gravity"], pr["clones"], pr["positions"], pr["obs_start"], pr["obs_clone"], pr["obs_z"], -1, True)
    ev = ref["gamma"] >= 0
    assert ev.sum() < n_feat          # the 1500-row cap is hit (Q13)
    assert np.allclose(got["gamma"][ev], ref["gamma"][ev], rtol=1e-7)
    assert np.array_equal((got["status"] >> 1) & 1, ref["passed"])
    assert got["rows"] == ref["rows"] > 1500
    # the oracle getter reconstructs the rotational parts of delta_x from quaternion differences (O(|dtheta|^2) accurate)
    assert np.allclose(got["delta_x"], ref["delta_x"], rtol=1e-5, atol=2e-8)
    Pg = s.ekf_get_cov()
    assert np.abs(Pg - ref["P"]).max() / np.abs(ref["P"]).max() < 1e-7
    s.close()


@pytest.mark.parametrize("models", [(1, 1), (1, 0)])
def test_equidistant_model_stereo_bit_exact(gpu_ctx, oracle, models):
    """Equidistant (fisheye) distortion model (image_processor.cpp:809-816,840): the stereo initial guess
    (undistort with R_cam0_cam1, distort into cam1), the epipolar gate and the published undistorted coordinates go
    through cv::fisheye-style undistort / distort with the deterministic atan / tan shared with the oracle."""
    w, h = 752, 480
    syn = oracle.Synth(seed=21, width=w, height=h)
    a1, b1 = syn.render(30)
    calib = oracle.euroc_calib(w, h)
    calib.cam0_model, calib.cam1_model = models
    fish = (-0.013, 0.021, -0.008, 0.0015)          # Kannala-Brandt k1..k4 of a mild fisheye
    for i in range(4):
        if models[0] == 1: calib.cam0_distortion[i] = fish[i]
        if models[1] == 1: calib.cam1_distortion[i] = fish[i] * 0.9
    fe = default_fe_cfg()
    s = capi.Stream(gpu_ctx, calib, fe, default_ekf_cfg())
    s.push_stereo(a1, b1)
    cand, _ = oracle.detect(a1)
    rng = np.random.default_rng(4)
    cand = np.concatenate([cand, np.stack([rng.uniform(0, w, 64), rng.uniform(0, h, 64)], 1).astype(np.float32)])
    got = s.track(cand, do_temporal=False)
    ref_c1, ref_in = oracle.stereo_match(calib, fe, a1, b1, cand)
    assert np.array_equal((got["status"] >> 1) & 1, ref_in)
    assert np.array_equal(got["out1"], ref_c1)
    K0, D0 = np.array(calib.cam0_intrinsics), np.array(calib.cam0_distortion)
    K1, D1 = np.array(calib.cam1_intrinsics), np.array(calib.cam1_distortion)
    assert np.array_equal(got["und0"], oracle.undistort(K0, D0, cand, model=models[0]))
    assert np.array_equal(got["und1"], oracle.undistort(K1, D1, ref_c1, model=models[1]))
    assert ref_in.sum() > 10
    s.close()


def test_track_capacity_and_errors(gpu_ctx, oracle):
    """Boundary behaviour of the C-ABI: capacity errors are reported, not crashed on."""
    s, calib = _stream(gpu_ctx, oracle, 376, 240)
    with pytest.raises(capi.MskfError):
        s.track(np.zeros((4, 2), np.float32), do_temporal=False)          # nothing pushed yet
    img = np.zeros((240, 376), np.uint8)
    s.push_stereo(img, img)
    res = s.track(np.zeros((0, 2), np.float32), do_temporal=False)       # empty input is fine
    assert len(res["status"]) == 0
    with pytest.raises(capi.MskfError):
        s.track(np.zeros((100000, 2), np.float32), do_temporal=False)    # exceeds the stream's point capacity
    with pytest.raises(capi.MskfError):
        s.push_stereo(np.zeros((100, 100), np.uint8), np.zeros((100, 100), np.uint8))   # wrong image size
    bad = oracle.euroc_calib(376, 240)
    bad.cam0_model = 7
    with pytest.raises(capi.MskfError):
        capi.Stream(gpu_ctx, bad, default_fe_cfg(), default_ekf_cfg())   # unknown distortion model
    s.close()


def _update_kwargs(pr, pair=False, **extra):
    """kwargs of Stream.ekf_update for a problem of ekf_problems, with arrays of their own (a test may spoil them)."""
    return dict(gravity=pr["gravity"].copy(), clones=pr["clones"].copy(), positions=pr["positions"].copy(), obs_start=pr["obs_start"].copy(),
                obs_clone=pr["obs_clone"].copy(), obs_z=pr["obs_z"].copy(), dof_offset=0 if pair else -1, apply_row_cap=not pair, **extra)


def _empty_kwargs(pr):
    return dict(gravity=pr["gravity"].copy(), clones=pr["clones"].copy(), positions=np.zeros((0, 3)), obs_start=np.zeros(1, np.int32),
                obs_clone=np.zeros(0, np.int32), obs_z=np.zeros((0, 4)), dof_offset=-1, apply_row_cap=True)


_MSKF_ERR_INVALID, _MSKF_ERR_CAPACITY = -1, -4
_REFUSAL_REF = {}


def _refusal_batch(calib):
    """Three streams of a 12-clone window: a pruning-shaped stack of 2250 rows (more than the 2048 rows a stream of this
    configuration starts with, so accepting it grows the stream's stacked-Jacobian buffer), a general one, a short one."""
    problems = [ekf_problems.make_problem(calib, seed=61, n_clones=12, n_feat=450, pair=(10, 11), noise=0.004),
                ekf_problems.make_problem(calib, seed=62, n_clones=12, n_feat=20),
                ekf_problems.make_problem(calib, seed=63, n_clones=12, n_feat=8)]
    return problems, [_update_kwargs(problems[0], pair=True), _update_kwargs(problems[1]), _update_kwargs(problems[2])]


# what is done to the middle stream's (mskf_ekf_update_args, buffers) before the batch is offered: buffers = (clones, features,
# obs_clone, obs_z, ...) as Stream._update_args returns them
def _spoil_n_clones(a, buf): a.n_clones -= 1
def _spoil_one_obs(a, buf): buf[1]["n_obs"][3] = 1
def _spoil_too_many_obs(a, buf): buf[1]["obs_start"][0] = 0; buf[1]["n_obs"][0] = 13          # max_cam_state_size is 12
def _spoil_obs_range(a, buf): a.n_obs -= 1                                                    # the last feature ends at n_obs
def _spoil_init_count(a, buf): buf[1]["needs_init"][2] = 1; buf[1]["n_init"][2] = 0
def _spoil_init_range(a, buf): buf[1]["needs_init"][2] = 1; buf[1]["init_start"][2] = a.n_obs - 1; buf[1]["n_init"][2] = 2
def _spoil_obs_clone(a, buf): buf[2][5] = 12
def _spoil_output(a, buf): a.delta_x = None


_EKF_REFUSALS = {
    "n_clones": (_spoil_n_clones, _MSKF_ERR_INVALID, "n_clones does not match the covariance dimension"),
    "one_observation": (_spoil_one_obs, _MSKF_ERR_INVALID, None),
    "more_observations_than_clones": (_spoil_too_many_obs, _MSKF_ERR_INVALID, None),
    "observations_past_n_obs": (_spoil_obs_range, _MSKF_ERR_INVALID, None),
    "init_count": (_spoil_init_count, _MSKF_ERR_INVALID, None),
    "init_range": (_spoil_init_range, _MSKF_ERR_INVALID, None),
    "obs_clone": (_spoil_obs_clone, _MSKF_ERR_INVALID, None),
    "missing_output": (_spoil_output, _MSKF_ERR_INVALID, None),
    "other_context": (None, _MSKF_ERR_INVALID, None),
    "too_many_rows": (None, _MSKF_ERR_CAPACITY, "stacked Jacobian exceeds the row capacity"),
}


@pytest.mark.parametrize("case", list(_EKF_REFUSALS))
def test_ekf_update_batch_refusals(gpu_ctx, oracle, case):
    """mskf_ekf_update_batch_begin refuses a batch whose MIDDLE stream is wrong (a valid stream before it, whose stack
    would grow its row buffer, and one after it): today's status code and message, no batch left pending (an _end is a
    no-op, the next _begin is accepted), and the same three streams then compute a valid batch bit-identically to three
    fresh streams.  Host-side refusals of bad arguments: nothing reaches the device."""
    import ctypes as C
    L = gpu_ctx.L
    L.mskf_ekf_update_batch_begin.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(capi.EkfUpdateArgs)]
    L.mskf_ekf_update_batch_end.argtypes = [C.c_void_p]
    calib = oracle.euroc_calib(376, 240)
    cfg = default_ekf_cfg(max_cam_state_size=12)
    problems, _ = _refusal_batch(calib)

    def fresh(ctx):
        ss = [capi.Stream(ctx, calib, default_fe_cfg(), cfg) for _ in problems]
        for s, pr in zip(ss, problems):
            s.ekf_set_cov(pr["P"])
        return ss

    def valid_batch(ss):
        got = gpu_ctx.ekf_update_batch(ss, _refusal_batch(calib)[1])
        return got, [s.ekf_get_cov() for s in ss]

    if not _REFUSAL_REF:
        ss = fresh(gpu_ctx)
        _REFUSAL_REF["got"], _REFUSAL_REF["P"] = valid_batch(ss)
        for s in ss:
            s.close()
        assert all(r["rows"] > 0 for r in _REFUSAL_REF["got"])
    ss = fresh(gpu_ctx)
    spoil, expect, message = _EKF_REFUSALS[case]
    kwargs = _refusal_batch(calib)[1]
    other = None
    handles = [s.h for s in ss]
    if case == "other_context":
        other = capi.Context(0)
        handles[1] = fresh(other)[1].h
    if case == "too_many_rows":           # 13108 two-observation features: 65540 rows > 65536
        n = 13108
        kwargs[1] = dict(kwargs[1], positions=np.zeros((n, 3)), obs_start=np.arange(0, 2 * n + 1, 2, dtype=np.int32),
                         obs_clone=np.tile(np.array([10, 11], np.int32), n), obs_z=np.zeros((2 * n, 4)), dof_offset=0, apply_row_cap=False)
    built = [capi.Stream._update_args(**kw) for kw in kwargs]
    if spoil is not None:
        spoil(built[1][0], built[1][1])
    for b in built:
        b[1][4][:] = 777.0                # delta_x: an _end that found something pending would overwrite it
    args = (capi.EkfUpdateArgs * 3)(*[b[0] for b in built])
    rc = L.mskf_ekf_update_batch_begin(gpu_ctx.h, 3, (C.c_void_p * 3)(*handles), args)
    assert rc == expect
    if message is not None:
        assert L.mskf_last_error().decode() == message
    assert L.mskf_ekf_update_batch_end(gpu_ctx.h) == 0
    assert all((b[1][4] == 777.0).all() for b in built) and all(b[1][7][0] == 0 for b in built)
    got, P = valid_batch(ss)              # (its _begin is accepted)
    for s in ss:
        s.close()
    if other is not None:
        other.close()
    for a, b, Pa, Pb in zip(got, _REFUSAL_REF["got"], P, _REFUSAL_REF["P"]):
        assert a["rows"] == b["rows"] and a["used_qr"] == b["used_qr"] and a["tiny_pivots"] == b["tiny_pivots"]
        assert np.array_equal(a["status"], b["status"]) and np.array_equal(a["gamma"], b["gamma"])
        assert np.array_equal(a["delta_x"], b["delta_x"]) and np.array_equal(Pa, Pb)


# Timed launches of one update batch per kind (mskf_ctx_get_timing), from DESIGN.md §2 and the comments of the launch chain:
#   FEATURES one slot around the pair kernels and the feature-block classes, whichever of them run;
#   SMALL    k_ekf_small_update, when some stream takes the small route (at most four clones touched);
#   when some stream takes the general route: GEMM<GRAM> and CHOL(0) if one of them compresses by Gram (modes 0, 1),
#   TSQR if one of them compresses by Householder (modes 2, 3), then GEMM<T>, GEMM<S2>, CHOL(1), TRSM;
#   GEMM<PUPD> for every batch that launches anything.  A batch without features launches nothing.
# The units are the algorithmic flops of each launch as integers, worked out from the problems' shapes
# outside the library: they pin what the entry point accounted before it was split into plan / grow / pack / enqueue.
_K_FEATURES, _K_TSQR, _K_GEMM, _K_CHOL, _K_TRSM, _K_SMALL, _K_COUNT = 5, 6, 7, 8, 9, 10, 14
_PAIR = dict(n_clones=12, n_feat=40, seed=71, pair=(10, 11), noise=0.004)
_PAIR2 = dict(n_clones=12, n_feat=25, seed=74, pair=(0, 1), noise=0.004)
_FEW = dict(n_clones=4, n_feat=10, seed=75)           # at most four clones touched, not a pair stack
_GEN, _GEN2 = dict(n_clones=12, n_feat=20, seed=72), dict(n_clones=12, n_feat=15, seed=73)
_GRAM_CHAIN = {_K_FEATURES: 1, _K_GEMM: 4, _K_CHOL: 2, _K_TRSM: 1}
_HH_CHAIN = {_K_FEATURES: 1, _K_TSQR: 1, _K_GEMM: 3, _K_CHOL: 1, _K_TRSM: 1}
_GRAM_UNITS = {_K_FEATURES: 28093452, _K_GEMM: 29216322, _K_CHOL: 1072476, _K_TRSM: 3217428}            # (_GEN, _GEN2), compressed by Gram
_HH_UNITS = {_K_FEATURES: 28093452, _K_TSQR: 16346610, _K_GEMM: 12869712, _K_CHOL: 536238, _K_TRSM: 3217428}     # ... by Householder
_EKF_CHAINS = {          # batch: [(problem | None = no features, compression_mode, triangulate)], launches per kind, units per kind
    "small_pairs": ([(_PAIR, 3, False), (_PAIR2, 3, False)], {_K_FEATURES: 1, _K_SMALL: 1, _K_GEMM: 1}, {_K_FEATURES: 5986500, _K_SMALL: 21172752}),
    "small_pairs_triangulated": ([(_PAIR, 3, True), (_PAIR2, 3, False)], {_K_FEATURES: 1, _K_SMALL: 1, _K_GEMM: 1}, {_K_FEATURES: 5986500, _K_SMALL: 21172752}),
    "small_not_pairs": ([(_FEW, 3, False)], {_K_FEATURES: 1, _K_SMALL: 1, _K_GEMM: 1}, {_K_FEATURES: 597144, _K_SMALL: 1310175}),
    "general_mode0": ([(_GEN, 0, False), (_GEN2, 0, False)], _GRAM_CHAIN, _GRAM_UNITS),
    "general_mode1": ([(_GEN, 1, False), (_GEN2, 1, False)], _GRAM_CHAIN, _GRAM_UNITS),
    "general_mode2": ([(_GEN, 2, False), (_GEN2, 2, False)], _HH_CHAIN, _HH_UNITS),
    "general_mode3": ([(_GEN, 3, False), (_GEN2, 3, False)], _HH_CHAIN, _HH_UNITS),
    "small_and_general": ([(_PAIR, 0, False), (_GEN, 0, False)], {**_GRAM_CHAIN, _K_SMALL: 1}, {_K_FEATURES: 19993464, _K_GEMM: 25358868, _K_CHOL: 1072476, _K_TRSM: 3217428}),
    "householder_and_gram": ([(_GEN, 3, False), (_GEN2, 0, False)], {**_GRAM_CHAIN, _K_TSQR: 1}, {**_GRAM_UNITS, _K_TSQR: 16346610}),
    "all_empty": ([(None, 3, False), (None, 0, False)], {}, {}),
    "some_empty": ([(None, 3, False), (_GEN, 0, False), (None, 0, False)], _GRAM_CHAIN, {_K_FEATURES: 16309464, _K_GEMM: 16000650, _K_CHOL: 536238, _K_TRSM: 1608714}),
}


@pytest.mark.parametrize("case", list(_EKF_CHAINS))
def test_ekf_update_launch_chain(gpu_ctx, oracle, case):
    """Which launches an update batch enqueues, by its composition: timing period 1, launches and units per kind."""
    import ctypes as C
    L = gpu_ctx.L
    L.mskf_ctx_set_timing.argtypes = [C.c_void_p, C.c_int]
    L.mskf_ctx_get_timing.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    calib = oracle.euroc_calib(376, 240)
    batch, launches, units = _EKF_CHAINS[case]
    base = ekf_problems.make_problem(calib, **_GEN)
    ss, kwargs, P0 = [], [], []
    for spec, mode, tri in batch:
        pr = base if spec is None else ekf_problems.make_problem(calib, **spec)
        s = capi.Stream(gpu_ctx, calib, default_fe_cfg(), default_ekf_cfg(max_cam_state_size=12, compression_mode=mode))
        s.ekf_set_cov(pr["P"])
        ss.append(s); P0.append(pr["P"])
        if spec is None:
            kwargs.append(_empty_kwargs(pr))
        else:
            kwargs.append(_update_kwargs(pr, pair="pair" in spec, **(dict(needs_init=np.ones(spec["n_feat"], np.int32)) if tri else {})))
    ms, n_l, n_u = np.zeros(_K_COUNT), np.zeros(_K_COUNT, np.int64), np.zeros(_K_COUNT, np.int64)
    assert L.mskf_ctx_set_timing(gpu_ctx.h, 1) == 0
    try:
        assert L.mskf_ctx_get_timing(gpu_ctx.h, ms.ctypes.data, n_l.ctypes.data, n_u.ctypes.data, 1) == 0      # reset
        got = gpu_ctx.ekf_update_batch(ss, kwargs)
        assert L.mskf_ctx_get_timing(gpu_ctx.h, ms.ctypes.data, n_l.ctypes.data, n_u.ctypes.data, 1) == 0
    finally:
        L.mskf_ctx_set_timing(gpu_ctx.h, 0)
    P1 = [s.ekf_get_cov() for s in ss]
    for s in ss:
        s.close()
    print("launch chain %s: launches %s units %s" % (case, {k: int(v) for k, v in enumerate(n_l) if v}, {k: int(v) for k, v in enumerate(n_u) if v}))
    assert {k: int(v) for k, v in enumerate(n_l) if v} == launches
    assert {k: int(v) for k, v in enumerate(n_u) if v} == units
    for (spec, _, _), r, Pa, Pb in zip(batch, got, P0, P1):
        if spec is not None:
            assert r["rows"] > 0
            continue
        # a stream without features: no correction, the covariance as it was; its position variances are read out behind
        # the others' updates when anything was launched, and "no value" (-1) when nothing ran
        assert r["rows"] == 0 and not r["delta_x"].any() and np.array_equal(Pa, Pb)
        assert np.array_equal(r["pos_var"], Pa[[12, 13, 14], [12, 13, 14]] if launches else np.full(3, -1.0))


@pytest.mark.parametrize("mode,expect", [(3, {1, 2}), (0, {0, 2})])
def test_ekf_mixed_batch_takes_each_stream_its_own_route(gpu_ctx, oracle, mode, expect):
    """One mskf_ekf_update_batch over streams of every route (EkfStreamDev::route): a pruning-shaped stream (pair kernels +
    fused small update), a stream whose features all have <= 4 observations (wave class), a general stream with small and
    large features, a stream with fewer stacked rows than active columns, an empty one.  Each stream's results are
    bit-identical to the same update issued alone."""
    calib = oracle.euroc_calib(376, 240)
    cfg = default_ekf_cfg(max_cam_state_size=30, compression_mode=mode)
    specs = [dict(n_clones=30, n_feat=120, seed=41, pair=(3, 4)),             # pairs + small
             dict(n_clones=30, n_feat=25, seed=42, min_obs=3, max_obs=4),     # wave class
             dict(n_clones=30, n_feat=50, seed=43, min_obs=3),                # general: classes [1] and [2]
             dict(n_clones=30, n_feat=2, seed=44, min_obs=3, max_obs=5),      # rows <= active columns
             dict(n_clones=12, n_feat=40, seed=45, pair=(10, 11))]            # another pair, another window size
    problems, kwargs = [], []
    for sp in specs:
        sp = dict(sp)
        max_obs = sp.pop("max_obs", None)
        pr = ekf_problems.make_problem(calib, **sp)
        if max_obs is not None:      # trim every feature to at most max_obs observations
            os_, oc, oz = [0], [], []
            for j in range(len(pr["obs_start"]) - 1):
                a, b = pr["obs_start"][j], min(pr["obs_start"][j + 1], pr["obs_start"][j] + max_obs)
                oc += list(pr["obs_clone"][a:b]); oz += list(pr["obs_z"][a:b]); os_.append(len(oc))
            pr["obs_start"], pr["obs_clone"], pr["obs_z"] = np.array(os_, np.int32), np.array(oc, np.int32), np.array(oz)
        pair = "pair" in sp
        problems.append(pr)
        kwargs.append(dict(gravity=pr["gravity"], clones=pr["clones"], positions=pr["positions"], obs_start=pr["obs_start"],
                           obs_clone=pr["obs_clone"], obs_z=pr["obs_z"], dof_offset=0 if pair else -1, apply_row_cap=not pair))
    def fresh():
        ss = [capi.Stream(gpu_ctx, calib, default_fe_cfg(), cfg) for _ in problems]
        for s, pr in zip(ss, problems):
            s.ekf_set_cov(pr["P"])
        return ss
    ss = fresh()
    alone = [s.ekf_update(**kw) for s, kw in zip(ss, kwargs)]
    P_alone = [s.ekf_get_cov() for s in ss]
    for s in ss:
        s.close()
    ss = fresh()
    together = gpu_ctx.ekf_update_batch(ss, kwargs)
    P_together = [s.ekf_get_cov() for s in ss]
    for s in ss:
        s.close()
    routes = set()
    for a, b, Pa, Pb in zip(alone, together, P_alone, P_together):
        assert a["rows"] == b["rows"] and a["used_qr"] == b["used_qr"]
        assert np.array_equal(a["status"], b["status"]) and np.array_equal(a["gamma"], b["gamma"])
        assert np.array_equal(a["delta_x"], b["delta_x"]) and np.array_equal(Pa, Pb)
        routes.add(a["used_qr"])
    assert all(r["rows"] > 0 for r in alone)
    assert expect <= routes                 # the batch really mixed compressed (1 Householder / 0 Gram) and uncompressed (2) updates
    # ... and against the oracle, per stream
    for pr, kw, got, Pg in zip(problems, kwargs, together, P_together):
        ref = oracle.ekf_update_problem(calib, cfg, pr["gravity"], pr["clones"], pr["P"], pr["positions"], pr["obs_start"], pr["obs_clone"],
                                        pr["obs_z"], kw["dof_offset"])
        assert np.array_equal((got["status"] >> 1) & 1, ref["passed"]) and got["rows"] == ref["rows"]
        assert np.abs(Pg - ref["P"]).max() / np.abs(ref["P"]).max() < 1e-8


def test_ekf_gated_out_block_leaves_a_gap_in_a_short_stack(gpu_ctx, oracle):
    """a stack with fewer STACKED rows than active columns whose last stacked row lies beyond them because a
    gated-out block sits in the middle (st <= na < me).  H^T H is singular by construction there, and the reference does
    not compress such a stack at all (msckf_vio.cpp:818-821): auto mode must not take the Gram path; the stacked rows are
    used as they are, addressed through a compact list of their indices (the gap does not fit the na-row work buffers).
    The middle feature is made an outlier (its observations pushed apart, alternately), which the gate rejects."""
    calib = oracle.euroc_calib(376, 240)
    cfg = default_ekf_cfg(max_cam_state_size=30)
    hit = 0
    for seed in range(300, 312):
        # three features seen by every clone; the first and the last are then cut down to five clones each (disjoint),
        # the middle one keeps all thirty: 17 + 17 stacked rows on 60 active columns, the last stacked row at 17 + 117 + 17
        full = ekf_problems.make_problem(calib, seed=seed, n_clones=30, n_feat=3, min_obs=30)
        keep = [np.arange(0, 5), np.arange(0, 30), np.arange(10, 15)]
        os_, oc, oz = [0], [], []
        for j in range(3):
            a = full["obs_start"][j]
            for k in keep[j]:
                oc.append(int(full["obs_clone"][a + k])); oz.append(full["obs_z"][a + k].copy())
            os_.append(len(oc))
        pr = dict(full, obs_start=np.array(os_, np.int32), obs_clone=np.array(oc, np.int32), obs_z=np.array(oz))
        a, b = pr["obs_start"][1], pr["obs_start"][2]
        pr["obs_z"][a:b] += 0.2 * np.where(np.arange(b - a) % 2 == 0, 1.0, -1.0)[:, None]      # the middle feature becomes a gross outlier
        ref = oracle.ekf_update_problem(calib, cfg, pr["gravity"], pr["clones"], pr["P"], pr["positions"], pr["obs_start"], pr["obs_clone"],
                                        pr["obs_z"], -1)
        if list(ref["passed"]) != [1, 0, 1]:
            continue
        n_obs = np.diff(pr["obs_start"])
        st, me = int((4 * n_obs[[0, 2]] - 3).sum()), int((4 * n_obs - 3).sum())
        used = sorted(set(int(c) for j in (0, 2) for c in pr["obs_clone"][pr["obs_start"][j]:pr["obs_start"][j + 1]]))
        na = 6 * len(used)
        assert st <= na < me
        hit += 1
        s = capi.Stream(gpu_ctx, calib, default_fe_cfg(), cfg)
        s.ekf_set_cov(pr["P"])
        got = s.ekf_update(pr["gravity"], pr["clones"], pr["positions"], pr["obs_start"], pr["obs_clone"], pr["obs_z"], -1, True)
        Pg = s.ekf_get_cov()
        s.close()
        assert got["rows"] == st == ref["rows"]
        assert got["used_qr"] == 2, "st <= na < me: the stacked rows are the measurement, uncompressed (never squared into H^T H)"
        assert np.abs(Pg - ref["P"]).max() / np.abs(ref["P"]).max() < 1e-11
        assert np.abs(got["delta_x"] - ref["delta_x"]).max() / np.abs(ref["delta_x"]).max() < 1e-9
    assert hit >= 2, "the oracle gated no [pass, reject, pass] case: widen the seed range"


def test_compression_mode_is_validated(gpu_ctx, oracle):
    """mskf_ekf_cfg.compression_mode took the place of padding: anything but 0, 1, 2, 3 is refused at stream creation."""
    calib = oracle.euroc_calib(376, 240)
    for bad in (-1, 4, 0x7fffffff):
        with pytest.raises(capi.MskfError):
            capi.Stream(gpu_ctx, calib, default_fe_cfg(), default_ekf_cfg(compression_mode=bad))


def _status(call, *a, **kw):
    """The mskf status a wrapper call ends with (0: accepted)."""
    try:
        call(*a, **kw)
        return 0
    except capi.MskfError as e:
        return e.code


def test_device_frame_entry_points_refuse_what_they_cannot_do(gpu_ctx, oracle):
    """mskf_fe_frame_batch_* (whole front-end frames on the device): no grid handed over yet, output arrays too small and
    per-cell limits above the kernels' bound are refused with a status and a message, never silently; the 2-point RANSAC
    configuration (refused until round 4, when the RANSAC moved from the host into the frame) is accepted."""
    from msckf_stereo_c_amd.ctypes_types import COMPAT_REFERENCE
    L = gpu_ctx.L
    w, h = 376, 240
    calib = oracle.euroc_calib(w, h)
    img = np.zeros((h, w), np.uint8)

    def frame(stream, cap):
        return _status(gpu_ctx.frame_batch_begin, [stream], [(img, img)], [dict(capacity=cap)])

    s = capi.Stream(gpu_ctx, calib, default_fe_cfg(), default_ekf_cfg())
    cap = s.grid_capacity()
    assert cap >= 4 * 5 * 4
    assert frame(s, cap) == -1 and b"no grid on the device" in L.mskf_last_error()          # MSKF_ERR_INVALID: first frame goes the phased way
    assert _status(s.set_grid) == 0
    assert frame(s, cap - 1) == -1                                                          # output arrays too small
    assert _status(s.set_grid, n=cap + 1) == -1
    s.close()
    s = capi.Stream(gpu_ctx, calib, default_fe_cfg(compat=COMPAT_REFERENCE & ~8), default_ekf_cfg())     # Q5 cleared: RANSAC on
    assert _status(s.set_grid) == 0
    assert frame(s, s.grid_capacity()) == 0                                                  # accepted: the RANSAC runs inside the frame
    assert _status(gpu_ctx.frame_batch_end) == 0
    s.close()
    s = capi.Stream(gpu_ctx, calib, default_fe_cfg(grid_min=17, grid_max=20), default_ekf_cfg())
    assert s.grid_capacity() == 0
    assert _status(s.set_grid) == -3
    s.close()


# ---- the front-end batches refuse before they touch anything (188 x 120: the size of tests/golden/frontend_188x120.npz)
_FE_W, _FE_H = 188, 120
_FE_REF = {}


def _fe_images(oracle):
    """Pair A and pair B of three streams: frames 0, 2, 4 and 6, 8, 10 of one synthetic sequence (the camera moves from frame 1 on)."""
    if "img" not in _FE_REF:
        syn = oracle.Synth(seed=0x5EED0090, width=_FE_W, height=_FE_H, n_static=1, n_loop=40)
        _FE_REF["img"] = ([syn.render(k) for k in (0, 2, 4)], [syn.render(k) for k in (6, 8, 10)])
        _FE_REF["calib"] = syn.calib
    return _FE_REF["img"] + (_FE_REF["calib"],)


def _fe_streams(ctx, calib, n=3, fe=None):
    return [capi.Stream(ctx, calib, fe or default_fe_cfg(), default_ekf_cfg()) for _ in range(n)]


def _push_state(s):
    """What a push leaves behind for one stream: the cell maxima, the four levels of cam0, and what a stereo-only track of the
    maxima above the detector threshold returns (it reads both pyramids)."""
    m = s.cell_maxima()
    top = m[m["score"] > s.fe_cfg.fast_threshold * 256]
    assert len(top) > 20
    trk = s.track(np.stack([top["x"], top["y"]], axis=1), do_temporal=0)
    return [m] + [s.get_level(1, l) for l in range(4)] + [trk[k] for k in ("out0", "out1", "und0", "und1", "status")]


def _same(a, b):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), i


@pytest.mark.parametrize("case", ["null_stream", "other_context", "null_cam1", "pending_track"])
def test_fe_push_batch_refusals(gpu_ctx, oracle, case):
    """mskf_fe_push_stereo_batch refuses a batch whose MIDDLE stream is wrong (a valid one before it) with MSKF_ERR_INVALID and
    has then changed nothing: maxima, pyramid levels and a repeated track of all three streams are bit-identical to what the
    accepted push of pair A left, and a valid push of pair B afterwards equals a fresh context that saw only A, then B."""
    A, B, calib = _fe_images(oracle)
    if "push" not in _FE_REF:
        ctx = capi.Context(0)
        ss = _fe_streams(ctx, calib)
        for pair in (A, B):
            ctx.push_stereo_batch(ss, [p[0] for p in pair], [p[1] for p in pair])
        _FE_REF["push"] = [[s.cell_maxima()] + [s.get_level(1, l) for l in range(4)] for s in ss]
        ctx.close()
    ss = _fe_streams(gpu_ctx, calib)
    gpu_ctx.push_stereo_batch(ss, [p[0] for p in A], [p[1] for p in A])
    before = [_push_state(s) for s in ss]
    # (the tracks above were batches of their own: the maxima of the push are still the context's latest)
    streams, cam0s, cam1s = list(ss), [p[0] for p in B], [p[1] for p in B]
    other = None
    if case == "null_stream":
        streams[1] = None
    elif case == "other_context":
        other = capi.Context(0)
        streams[1] = _fe_streams(other, calib, 1)[0]
    elif case == "null_cam1":
        cam1s[1] = None
    elif case == "pending_track":
        gpu_ctx.track_batch_begin(ss[2:], [dict(pts=np.array([[40.0, 40.0], [90.0, 60.0]]), do_temporal=0)])
    try:
        assert _status(gpu_ctx.push_stereo_batch, streams, cam0s, cam1s) == _MSKF_ERR_INVALID
    finally:
        gpu_ctx.track_batch_end()
        if other is not None:
            other.close()
    for s, want in zip(ss, before):
        _same(_push_state(s), want)
    gpu_ctx.push_stereo_batch(ss, [p[0] for p in B], [p[1] for p in B])
    for s, want in zip(ss, _FE_REF["push"]):
        _same([s.cell_maxima()] + [s.get_level(1, l) for l in range(4)], want)
    for s in ss:
        s.close()


_FRAME_KEYS = ("id", "lifetime", "cam0", "cam1", "und0", "und1")
_FRAME_COUNTS = ("n", "before_tracking", "after_tracking", "after_matching", "after_ransac", "n_candidates", "n_new", "next_feature_id", "ransac_draws")


def _same_frames(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert [g[k] for k in _FRAME_COUNTS] == [w[k] for k in _FRAME_COUNTS]
        _same([g[k] for k in _FRAME_KEYS], [w[k] for k in _FRAME_KEYS])


def _frame(ctx, ss, pairs, args=None):
    ctx.frame_batch_begin(ss, pairs, args or [{} for _ in ss])
    return ctx.frame_batch_end()


@pytest.mark.parametrize("case,expect", [("grid_never_set", _MSKF_ERR_INVALID), ("capacity_too_small", _MSKF_ERR_INVALID), ("null_cam0", _MSKF_ERR_INVALID),
                                         ("pending_track", _MSKF_ERR_INVALID)])
def test_fe_frame_batch_refusals(gpu_ctx, oracle, case, expect):
    """mskf_fe_frame_batch_begin refuses a batch whose MIDDLE stream is wrong with today's status and has then changed nothing:
    the same three streams run the next frame bit-identically to three streams on another context that were never offered
    the refused batch (grid, ids, lifetimes, points, counters, id counter, RANSAC draw counter)."""
    A, B, calib = _fe_images(oracle)
    other = capi.Context(0)
    sets, first = [], []
    for ctx in (gpu_ctx, other):
        ss = _fe_streams(ctx, calib)
        for s in ss:
            s.set_grid()
        first.append(_frame(ctx, ss, A))
        sets.append(ss)
    assert all(r["n"] > 0 for r in first[0])
    _same_frames(first[0], first[1])
    ss = sets[0]
    extra = _fe_streams(gpu_ctx, calib, 1)[0]               # a stream of the context whose grid was never set
    streams, pairs, args = list(ss), list(B), [{} for _ in ss]
    if case == "grid_never_set":
        streams[1] = extra
    elif case == "capacity_too_small":
        args[1] = dict(capacity=ss[1].grid_capacity() - 1)
    elif case == "null_cam0":
        pairs[1] = (None, B[1][1])
    elif case == "pending_track":
        extra.push_stereo(*A[0])
        gpu_ctx.track_batch_begin([extra], [dict(pts=np.array([[40.0, 40.0], [90.0, 60.0]]), do_temporal=0)])
    try:
        assert _status(gpu_ctx.frame_batch_begin, streams, pairs, args) == expect
        assert _status(gpu_ctx.frame_batch_end) == 0         # nothing pending
    finally:
        gpu_ctx.track_batch_end()
    got, want = _frame(gpu_ctx, sets[0], B), _frame(other, sets[1], B)
    assert all(r["n"] > 0 for r in want)
    _same_frames(got, want)
    extra.close()
    for s in sets[0]:
        s.close()
    other.close()


def test_fe_frame_batch_mixed_capacities(gpu_ctx, oracle):
    """One frame batch of two streams whose grid configurations, hence capacities and export blocks, differ: over three frames
    every output of each stream equals, bit for bit, the same stream run alone on a context of its own."""
    syn = oracle.Synth(seed=0x5EED0091, width=_FE_W, height=_FE_H, n_static=1, n_loop=40)
    cfgs = [default_fe_cfg(), default_fe_cfg(grid_row=3, grid_col=6, grid_min=2, grid_max=6)]      # (the oracle's front-end keeps 60 and 36 features on these frames)
    frames = [syn.render(k) for k in (0, 2, 4)]
    ss = [_fe_streams(gpu_ctx, syn.calib, 1, fe)[0] for fe in cfgs]
    assert ss[0].grid_capacity() != ss[1].grid_capacity() and min(s.grid_capacity() for s in ss) > 0
    for s in ss:
        s.set_grid()
    batch = [_frame(gpu_ctx, ss, [f, f]) for f in frames]
    for i, fe in enumerate(cfgs):
        ctx = capi.Context(0)
        s = _fe_streams(ctx, syn.calib, 1, fe)[0]
        s.set_grid()
        for k, f in enumerate(frames):
            alone = _frame(ctx, [s], [f])
            assert alone[0]["n"] > 0
            _same_frames([batch[k][i]], alone)
        ctx.close()
    for s in ss:
        s.close()
