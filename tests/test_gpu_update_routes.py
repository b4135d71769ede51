"""The dense half of the measurement update on the device (k_ekf_gemm<GRAM|T|S2|PUPD>, k_ekf_chol_lds, k_ekf_chol,
k_ekf_tsqr<32,2,2> / <16,4,2>, k_ekf_trsm, k_ekf_small_update, tsqr_wide<4,12|8|4> in ekf_compress_exit) at every size limit
the code branches on, against the long-double reference of tests/update_cases.py.

tests/test_update_cases.py shows on the CPU that every case reaches the branch it is named for, that its gate and bias
margins hold, that the bars can be met in double arithmetic (the oracle and a numpy Gram update stay within one eighth of
them) and that the reference notices five kinds of mistakes at 100 times the bars.

Bars (update_cases.py), all taken from the project and not widened here:
  Householder and uncompressed routes : D_P < 1e-12, D_x < 1e-9 against the plain long-double update;
  Gram route                          : D_P, D_x < 1e-9 against update_with_prior (G + lambda I stated exactly), D_P < 1e-6
                                        (QR_BIAS_LIMIT) against the plain update.
D_P = max|dP| / max|P_ref|, D_x = max|d delta_x| / max|delta_x_ref|.  A device result beyond a bar, on a case the CPU file
accepted, is a finding.  Every test prints its figures; measured on an MI355X (per family: DESIGN.md section 1):
  Householder and uncompressed routes : D_P <= 6.0e-14 (fallback_w30_m0; 2.0e-15 without the bias-forced problems), D_x <= 9.9e-13;
  Gram route                          : D_P <= 2.0e-14, D_x <= 1.9e-13 against update_with_prior; D_P <= 2.3e-10 against the plain update.
The bias-forced problems (update_cases.FORCED) carry one prior variance of 1e4 that dominates max|P|: they are judged a
second time on P' and delta_x without that state's row and column.
"""
import numpy as np
import pytest

from msckf_stereo_c_amd import capi
from msckf_stereo_c_amd.ctypes_types import default_ekf_cfg, default_fe_cfg

import feature_reference as FR
import update_cases as U

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not FR.HAVE_LONG_DOUBLE, reason=FR.NEED_LONG_DOUBLE)]

ALL = sorted(U.CASES)


def _kwargs(c):
    return dict(gravity=c["gravity"].copy(), clones=c["clones"].copy(), positions=c["positions"].copy(), obs_start=c["obs_start"].copy(),
                obs_clone=c["obs_clone"].copy(), obs_z=c["obs_z"].copy(), dof_offset=c["dof_offset"], apply_row_cap=c["apply_row_cap"])


def _empty_kwargs(c):
    return dict(gravity=c["gravity"].copy(), clones=c["clones"].copy(), positions=np.zeros((0, 3)), obs_start=np.zeros(1, np.int32),
                obs_clone=np.zeros(0, np.int32), obs_z=np.zeros((0, 4)), dof_offset=-1, apply_row_cap=True)


def _stream(ctx, c):
    s = capi.Stream(ctx, c["calib"], default_fe_cfg(), default_ekf_cfg(max_cam_state_size=c["window"], compression_mode=c["mode"]))
    s.ekf_set_cov(c["P"])
    return s


def _run(ctx, c):
    """One stream, ekf_set_cov, one ekf_update -> (result dict, P')."""
    s = _stream(ctx, c)
    got = s.ekf_update(**_kwargs(c))
    Pg = s.ekf_get_cov()
    s.close()
    return got, Pg


def _same_bits(a, Pa, b, Pb):
    assert a["rows"] == b["rows"] and a["used_qr"] == b["used_qr"]
    assert np.array_equal(a["status"], b["status"])
    assert np.array_equal(a["gamma"].view(np.uint64), b["gamma"].view(np.uint64))
    assert np.array_equal(a["delta_x"].view(np.uint64), b["delta_x"].view(np.uint64))
    assert np.array_equal(Pa.view(np.uint64), Pb.view(np.uint64))


def _check(c, got, Pg):
    s = U.stack(c["problem"])
    assert got["rows"] == c["st"]
    assert np.array_equal(got["status"] & 1, np.ones(len(c["specs"]), np.uint8))          # positions given: valid
    assert np.array_equal(((got["status"] >> 1) & 1).astype(bool), s["passed"])
    assert got["used_qr"] == c["used_qr"]
    assert np.array_equal(Pg.view(np.uint64), Pg.T.copy().view(np.uint64))
    plain = U.reference(c["problem"])
    D_P, D_x = U.distances(got["delta_x"], Pg, plain)
    bar = U.GRAM_BAR if c["gram"] else U.HH_P_BAR
    min_eig = float(np.linalg.eigvalsh(Pg).min()) / float(np.abs(c["P"]).max())
    line = "%s (%s, mode %d, used_qr %d): against the plain reference D_P %.3e, D_x %.3e" % (c["name"], c["limit"], c["mode"], got["used_qr"], D_P, D_x)
    if c["gram"]:
        G_P, G_x = U.distances(got["delta_x"], Pg, U.reference_with_prior(c["problem"]))
        line += " (bar %.0e for D_P); against update_with_prior D_P %.3e, D_x %.3e (bar %.0e)" % (U.GRAM_PLAIN_BAR, G_P, G_x, U.GRAM_BAR)
    else:
        line += " (bars %.0e, %.0e)" % (U.HH_P_BAR, U.HH_X_BAR)
    B_P = B_x = 0.0
    if c["inflated"] is not None:
        B_P, B_x = U.distances(got["delta_x"], Pg, plain, exclude=c["inflated"])
        line += "; without state %d D_P %.3e, D_x %.3e" % (c["inflated"], B_P, B_x)
    print(line + "; min eig(P') / max|P| %.3e" % min_eig)
    if c["gram"]:
        assert G_P < U.GRAM_BAR and G_x < U.GRAM_BAR
        assert D_P < U.GRAM_PLAIN_BAR
    else:
        assert D_P < U.HH_P_BAR and D_x < U.HH_X_BAR
        assert B_P < U.HH_P_BAR and B_x < U.HH_X_BAR
    assert min_eig >= -bar


@pytest.mark.parametrize("name", ALL)
def test_route(gpu_ctx, name):
    """One case of update_cases.CASES: rows, status bits, used_qr, the distances, bitwise symmetry, min eig(P'); and the same
    update on a second fresh stream gives identical bits (the sums run in a fixed order, no atomics)."""
    c = U.case(name)
    got, Pg = _run(gpu_ctx, c)
    _check(c, got, Pg)
    again, P_again = _run(gpu_ctx, c)
    _same_bits(got, Pg, again, P_again)


def test_fallback_row_block_does_not_depend_on_the_batch(gpu_ctx):
    """The 31-clone stream whose bias flag sends it to the fallback TSQR of k_ekf_chol, alone and beside a 64-clone stream.  The
    launch's panel is sized for the widest stream of the batch (16 x 400 doubles beside W = 64, 16 x 192 alone); a row block
    sized from it would be 32 rows beside the wide stream (6400 >= 32 x 187) and 16 alone, and the two orders of summation differ
    in the last bits.  The block is sized from the stream's own dimension: identical bits (EkfStreamDev::route's promise, "a
    stream's arithmetic does not depend on its neighbours")."""
    c, wide = U.case("chol_w31_bias_m0"), U.case("big_w64_m1")
    assert U.chol_class(c["window"]) == U.chol_class(wide["window"]) == 1
    assert U.wide_rows_per_lane(c["window"], c["n1"]) == 4 and U.LNB * ((wide["n1"] + 15) // 16 * 16) >= 32 * c["n1"]
    alone, P_alone = _run(gpu_ctx, c)
    ss = [_stream(gpu_ctx, c), _stream(gpu_ctx, wide)]
    together = gpu_ctx.ekf_update_batch(ss, [_kwargs(c), _kwargs(wide)])
    P_together = [s.ekf_get_cov() for s in ss]
    for s in ss:
        s.close()
    assert alone["used_qr"] == together[0]["used_qr"] == 1 and together[1]["used_qr"] == 0
    _check(c, together[0], P_together[0])
    _check(wide, together[1], P_together[1])
    _same_bits(alone, P_alone, together[0], P_together[0])


BATCH = ["chol_w30_m1", "chol_w31_m1", "tsqr_w42_k257_m3", "tsqr_w43_k273_m3", "trsm_w35_m3", "small4_w30_k598_m3"]


def test_batch_of_every_class_is_bitwise_the_updates_alone(gpu_ctx):
    """One mskf_ekf_update_batch over W = 30 and W = 31 in mode 1, W = 42, W = 43 and W = 35 in mode 3, a small-route stream
    and an empty one: both factorisation kernels, both k_ekf_tsqr instantiations and both paths of k_ekf_trsm (n = 180 beside
    n = 210 and more) in single launches with the class filters live.  Every stream's status, gamma, delta_x, rows, used_qr and P'
    are bitwise those of the same update alone."""
    cases = [U.case(n) for n in BATCH]
    assert {U.chol_class(c["window"]) for c in cases if c["route"] == "general"} == {0, 1}
    assert {U.tsqr_class(c["window"]) for c in cases if c["route"] == "general" and c["mode"] == 3} == {0, 1}
    assert {U.l_fits(c["na"]) for c in cases if c["route"] == "general"} == {True, False}
    assert any(c["route"] == "small" for c in cases)
    alone = [_run(gpu_ctx, c) for c in cases]
    empty = dict(cases[0], mode=3)
    ss = [_stream(gpu_ctx, c) for c in cases] + [_stream(gpu_ctx, empty)]
    together = gpu_ctx.ekf_update_batch(ss, [_kwargs(c) for c in cases] + [_empty_kwargs(empty)])
    P_together = [s.ekf_get_cov() for s in ss]
    for s in ss:
        s.close()
    for c, (a, Pa), b, Pb in zip(cases, alone, together, P_together):
        _same_bits(a, Pa, b, Pb)
        _check(c, b, Pb)
    assert together[-1]["rows"] == 0 and not together[-1]["delta_x"].any()
    assert np.array_equal(P_together[-1], np.ascontiguousarray(empty["P"]))
