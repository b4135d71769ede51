"""The measurement update's per-feature stage on the device (triangulate_wave, k_ekf_triangulate, the three instantiations of
k_ekf_feature_blocks, k_ekf_pair_blocks) at its triangulation, validity and size-class edges, against the long-double
reference of tests/feature_reference.py.

The cases are those of tests/feature_cases.py; tests/test_feature_cases.py shows on the CPU that they reach what they are
named for, that no feature has to be excluded, where the two bars TRI_BAR and GAMMA_BAR come from (eight times the
double-precision oracle's own difference from the reference) and that the reference notices each of six deliberate mistakes.

Every case gets the same check (_check): valid bits exactly, the triangulated positions in inverse-depth coordinates within
TRI_BAR (world coordinates cannot hold a relative bar at 100 m and more), gamma at the device's own positions within
GAMMA_BAR, pass bits exactly, the stacked rows, and delta_x / P against the oracle's update of the valid features alone at
the bars of test_ekf_update_matches_oracle: an invalid feature must leave no trace in the update.

The observations are laid out as buildPruneUpdate (host/msckf_vio.cpp) lays them out: a feature's triangulation
observations first, its Jacobian observations behind them, so init_start != obs_start and n_init != n_obs throughout.
"""
import ctypes as C

import numpy as np
import pytest

from msckf_stereo_c_amd import capi
from msckf_stereo_c_amd.ctypes_types import default_ekf_cfg, default_fe_cfg

import feature_cases as FC
import feature_reference as FR
from test_feature_cases import GAMMA_BAR, SIGMA2, TRI_BAR

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not FR.HAVE_LONG_DOUBLE, reason=FR.NEED_LONG_DOUBLE)]


def _args(c):
    """(mskf_ekf_update_args, buffers, result builder) of a case in its device layout."""
    d = c["dev"]
    n = len(c["cls"])
    a, keep, result = capi.Stream._update_args(c["gravity"], c["clones"], c["positions"], np.zeros(n + 1, np.int32), d["obs_clone"], d["obs_z"],
                                               c["dof_offset"], c["apply_row_cap"], needs_init=c["needs_init"], init_ranges=d["init_ranges"])
    feats = keep[1]
    feats["obs_start"], feats["n_obs"] = d["obs_start"], d["n_obs"]        # the Jacobian ranges are not back to back
    return a, keep, result


def _stream(ctx, c):
    s = capi.Stream(ctx, c["calib"], default_fe_cfg(), default_ekf_cfg(max_cam_state_size=c["window"]))
    s.ekf_set_cov(c["P"])
    return s


def _run(ctx, c):
    s = _stream(ctx, c)
    a, keep, result = _args(c)
    capi._chk(s.L.mskf_ekf_update(s.h, C.byref(a)))
    got = result()
    Pg = s.ekf_get_cov()
    s.close()
    return got, Pg


def _run_batch(ctx, cases):
    ss = [_stream(ctx, c) for c in cases]
    built = [_args(c) for c in cases]
    n = len(cases)
    args = (capi.EkfUpdateArgs * n)(*[b[0] for b in built])
    hs = (C.c_void_p * n)(*[s.h for s in ss])
    ctx.L.mskf_ekf_update_batch.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(capi.EkfUpdateArgs)]
    capi._chk(ctx.L.mskf_ekf_update_batch(ctx.h, n, hs, args))
    out = [(b[2](), s.ekf_get_cov()) for b, s in zip(built, ss)]
    for s in ss:
        s.close()
    return out


def _check(name, got, Pg, oracle):
    c = FC.case(name)
    chi2 = FR.chi2_table()
    n = len(c["cls"])
    tri = FC.reference_triangulation(name)
    valid = np.array([True if t is None else t["valid"] for t in tri])
    init = c["needs_init"].astype(bool)
    status = got["status"]
    assert np.array_equal(status & 1, valid.astype(np.uint8))
    assert (status[~valid] == 0).all() and (got["gamma"][~valid] == -1.0).all()
    assert np.array_equal(got["positions"][~init], c["positions"][~init])          # given positions come back as they went in
    d_tri = 0.0
    for j in np.flatnonzero(init & valid):
        sol = FR.to_inverse_depth(c["clones"], c["init_clone"][c["init_start"][j]], got["positions"][j])
        d_tri = max(d_tri, float(np.abs(sol - tri[j]["solution"]).max()))
    keep = np.flatnonzero(valid)
    g_ref, p_ref = FC.reference_gates(c, got["positions"], SIGMA2, chi2, only=keep)
    rel = np.abs(got["gamma"][keep] - g_ref[keep]) / g_ref[keep]
    d_gamma, worst = float(rel.max()), int(keep[int(np.argmax(rel))])
    print("%s: device against long-double reference: |d(alpha, beta, rho)| %.3e (bar %.1e), relative gamma %.3e (bar %.1e; feature %d, "
          "%d observations: device %.17g, reference %.17g)" % (name, d_tri, TRI_BAR, d_gamma, GAMMA_BAR, worst, len(c["specs"][worst]["jac"]),
                                                            got["gamma"][worst], float(g_ref[worst])))
    assert d_tri <= TRI_BAR
    assert d_gamma <= GAMMA_BAR
    # the gate's verdict of every feature is the reference's; behind the row cap the device clears the bit of a block it does
    # not stack (ekf_cap.h): the first passing feature whose rows take the stack beyond max_stack_rows is the last one stacked
    rows_of = np.array([4 * len(s["jac"]) - 3 for s in c["specs"]])
    stacked = p_ref.copy()
    total = int(rows_of[p_ref].sum())
    if c["apply_row_cap"]:
        beyond = np.flatnonzero(np.cumsum(np.where(p_ref, rows_of, 0)) > default_ekf_cfg().max_stack_rows)
        if len(beyond):
            stacked[beyond[0] + 1:] = False
    capped = int(rows_of[stacked].sum()) < total
    assert np.array_equal(((status >> 1) & 1).astype(bool), stacked)
    # the update: the oracle on the valid features alone, at the device's positions
    orc = FC.oracle_update(oracle, c, got["positions"], keep)
    assert total > 0
    assert got["rows"] == orc["rows"] == int(rows_of[stacked].sum())
    assert capped == (bool(c["apply_row_cap"]) and bool((orc["gamma"][keep] < 0).any()))
    if capped:
        assert got["rows"] > default_ekf_cfg().max_stack_rows
    scale = np.abs(orc["delta_x"]).max()
    assert np.allclose(got["delta_x"], orc["delta_x"], rtol=1e-6, atol=1e-9 * max(scale, 1e-3))
    assert np.allclose(Pg, orc["P"], rtol=1e-7, atol=1e-8 * np.abs(orc["P"]).max())
    assert np.array_equal(Pg, Pg.T)
    return d_tri, d_gamma


PAIR = ["pair_w12_65", "pair_w64_129"]
WAVE = ["wave_w12_5", "wave_w30_65", "wave_w64_257"]
SMALL = ["small_w30"]
BIG = ["big_w30", "big_w32", "big_w64"]
SLOTS = ["slots_small_65", "slots_small_129", "slots_big_65", "slots_big_129"]


@pytest.mark.parametrize("name", PAIR)
def test_pair_route(gpu_ctx, oracle, name):
    """k_ekf_triangulate + k_ekf_pair_blocks: n_init in {1, 2, 3, 32, 33, 64} in front of the two Jacobian observations,
    given and triangulated positions mixed, far features with invalid results (feature 0, feature 64 and the last among
    them), 65 and 129 features."""
    c = FC.case(name)
    assert c["variant"] == "pair" and c["dof_offset"] == 0
    got, Pg = _run(gpu_ctx, c)
    _check(name, got, Pg, oracle)
    assert got["status"][0] == 0 and got["status"][64] == 0 and (name != "pair_w64_129" or got["status"][128] == 0)


@pytest.mark.parametrize("name", WAVE)
def test_wave_route(gpu_ctx, oracle, name):
    """k_ekf_feature_blocks<4, true, 256>: 2, 3 and 4 observations over differing clones, triangulations over n_obs, 5, 16,
    17 and 32 clones, far features with invalid results; 5, 65 and 257 features leave one wavefront of the last workgroup
    with work."""
    c = FC.case(name)
    assert c["variant"] == "wave"
    got, Pg = _run(gpu_ctx, c)
    _check(name, got, Pg, oracle)


def test_wave_route_wide_stereo(gpu_ctx, oracle):
    """cam1 turned by 75 degrees about y: features on one side lie in front of every cam0 and behind every cam1, so the valid
    bit has to look at the cam1 views.  A feature close to cam1's image plane has Jacobian entries in the thousands (the largest
    singular value of feature 7's H_f is 4640): a gate that forms H_xj P H_xj^T first and reflects it afterwards loses
    |H_xj P H_xj^T| / |S_g| of its digits.  The wave variant did (gamma of feature 7 was 9.4e-9 off, bar 3.7e-12) and now forms
    S_g = H_o P_cc H_o^T from the projected block, as the pair kernel and the oracle do."""
    c = FC.case("wide_stereo_w12")
    assert c["variant"] == "wave"
    got, Pg = _run(gpu_ctx, c)
    _check("wide_stereo_w12", got, Pg, oracle)


def test_one_large_triangulation_takes_the_stream_off_the_wave_route(gpu_ctx, oracle):
    """The 257-feature stream with one triangulation over 33 clones: its features go to the small and the big class, with the
    same results to the bars; every other feature's verdict is the wave route's."""
    wave, _ = _run(gpu_ctx, FC.case("wave_w64_257"))
    c = FC.case("wave_w64_257_leaves")
    assert c["variant"] == "mixed" and set(c["cls"]) == {"small", "big"}
    got, Pg = _run(gpu_ctx, c)
    _check("wave_w64_257_leaves", got, Pg, oracle)
    others = np.arange(len(c["cls"])) != 100
    assert np.array_equal(got["status"][others], wave["status"][others])


@pytest.mark.parametrize("name", SMALL + BIG)
def test_size_classes(gpu_ctx, oracle, name):
    """k_ekf_feature_blocks<16, false, 64> (5 and 16 observations, 5 with a triangulation over 16), <32, false, 256> (17, 30,
    31, 32 in a 32-clone window, 17, 29, 30 in a 30-clone one) and <64, false, 256> (33, 63, 64, and 30 / 31 again), 5
    observations with a triangulation over 17 clones in the big class; passing, gated-out and invalid features on both sides
    of the 120-row boundary between the gate matrix in LDS and in global memory."""
    c = FC.case(name)
    assert c["variant"] == "mixed"
    got, Pg = _run(gpu_ctx, c)
    _check(name, got, Pg, oracle)


@pytest.mark.parametrize("name", SLOTS)
def test_slot_loops(gpu_ctx, oracle, name):
    """65 and 129 members of one class in one stream: a group handles two or three features in turn, after an invalid, a
    passing or a gated-out one (test_feature_cases.test_slot_patterns), and reuses its gate slot in global memory (31
    observations).  The row cap stops the oracle; every feature's gamma and bits are the reference's."""
    c = FC.case(name)
    assert len(set(c["cls"])) == 1 and c["apply_row_cap"]
    got, Pg = _run(gpu_ctx, c)
    _check(name, got, Pg, oracle)


def test_instantiation_does_not_change_a_streams_result(gpu_ctx, oracle):
    """A 30-clone-window stream with big-class features alone (k_ekf_feature_blocks<32, ...>) and beside a 64-clone-window
    stream (<64, ...>, chosen by the largest window of the batch): bit-identical, as plan_stream promises."""
    a, b = FC.case("big_w30"), FC.case("big_w64")
    assert set(a["cls"]) == {"big"}
    alone, P_alone = _run(gpu_ctx, a)
    (mixed, P_mixed), (other, P_other) = _run_batch(gpu_ctx, [a, b])
    _check("big_w64", other, P_other, oracle)
    assert np.array_equal(alone["status"], mixed["status"])
    assert np.array_equal(alone["gamma"].view(np.uint64), mixed["gamma"].view(np.uint64))
    assert np.array_equal(alone["positions"].view(np.uint64), mixed["positions"].view(np.uint64))
    assert alone["rows"] == mixed["rows"]
    assert np.array_equal(alone["delta_x"].view(np.uint64), mixed["delta_x"].view(np.uint64))
    assert np.array_equal(P_alone.view(np.uint64), P_mixed.view(np.uint64))
