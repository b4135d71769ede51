"""tests/update_cases.py mirrors the limits the dense update kernels branch on; csrc/hip/ekf_limits.h is where the host and the
kernels take them from.  The header (plain C++) is compiled with g++ into a program that prints it (tests/cpp/
ekf_limits_test.cpp), and the mirror is held against the print-out: the constants, chol_class / tsqr_class on every window
4..64, l_fits on every n, `predicted` against the header's two compression predicates on every input, and the public meaning of
diag_out against the header's decode of the diagnostics word.  Nothing here reads the device."""
import os
import subprocess

import pytest

import update_cases as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def header(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ekf_limits") / "ekf_limits_test")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", ROOT, "-o", exe, os.path.join(ROOT, "tests", "cpp", "ekf_limits_test.cpp")])
    out = {"class": {}, "l_fits": {}, "redo": {}, "direct": {}, "decode": {}, "value": {}}
    for line in subprocess.check_output([exe], text=True).splitlines():
        f = line.split()
        if f[0] == "class":
            out["class"][int(f[1])] = (int(f[2]), int(f[3]))
        elif f[0] == "l_fits":
            out["l_fits"][int(f[1])] = bool(int(f[2]))
        elif f[0] in ("redo", "direct"):
            out[f[0]][tuple(int(x) for x in f[1:-1])] = bool(int(f[-1]))
        elif f[0] == "decode":
            out["decode"][int(f[1])] = tuple(int(x) for x in f[2:])
        else:
            out["value"][f[0]] = float(f[1])
    return out


def test_constants_are_the_headers(header):
    mirror = {"EKF_IMU_DIM": U.IMU_DIM, "SU_MAX_NA": U.SU_MAX_NA, "SU_CH": U.SU_CH, "CHOL_LDS_MAX_ROWS": U.CHOL_LDS_MAX_ROWS, "CHOL_PAN_RS": U.CHOL_PAN_RS,
              "TQ_THREADS": U.TQ_THREADS, "TS_RB": U.TS_RB, "TS_LPF": U.TRSM_LPF, "EKF_GEMM_TILE": U.GEMM_TILE, "QR_BIAS_LIMIT": U.QR_BIAS_LIMIT}
    for name, value in mirror.items():
        assert header["value"][name] == value, name
    assert header["value"]["EKF_ROWS_COUNT"] == 5


def test_class_functions_agree_on_every_window(header):
    assert sorted(header["class"]) == list(range(4, 65))
    for w, (chol, tsqr) in header["class"].items():
        assert (U.chol_class(w), U.tsqr_class(w)) == (chol, tsqr), w
    assert sorted(header["l_fits"]) == list(range(1, 6 * 64 + 1))
    for n, fits in header["l_fits"].items():
        assert U.l_fits(n) == fits, n
    # both sides of every limit are among the windows asked
    assert {c for c, _ in header["class"].values()} == {0, 1} == {t for _, t in header["class"].values()} == {int(v) for v in header["l_fits"].values()}


def test_predicted_is_the_headers_decision(header):
    """used_qr of a stream: the general route leaves a stack the header calls direct uncompressed and has a Gram factor whenever
    it asks; the small route compresses every stack and has a Gram factor to use only when st > na."""
    na = 24
    for mode in range(4):
        for st in (na - 1, na, na + 1):
            for bias in (False, True):
                general = 2 if header["direct"][(mode, st)] else int(header["redo"][(mode, 1, int(bias))])
                small = int(header["redo"][(mode, int(st > na), int(bias))])
                assert U.predicted("general", mode, st, na, bias) == general, (mode, st, bias)
                assert U.predicted("small", mode, st, na, bias) == small, (mode, st, bias)


def test_diag_out_keeps_its_public_meaning(header):
    """diag_out[0] = 0 Gram factor / 1 Householder / 2 uncompressed, diag_out[1] = the tiny-pivot count; then the bias bit."""
    assert header["decode"] == {0: (0, 0, 0), 1: (1, 0, 0), 4: (2, 0, 0), 2: (0, 0, 1), 3: (1, 0, 1), 3 << 8: (0, 3, 0),
                                (7 << 8) | 3: (1, 7, 1), (300 << 8) | 2: (0, 300, 1)}
