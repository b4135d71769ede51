"""measurementJacobian (msckf_vio.cpp:610-677): the DEVICE source (csrc/hip/ekf_meas.h, what k_ekf_feature_blocks,
k_ekf_pair_blocks and the host's Jacobian dump all run) executed on the CPU == the oracle's MsckfVio::measurementJacobian,
value for value."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ekf_problems
from msckf_stereo_c_amd.ctypes_types import Calib, default_ekf_cfg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MUTATIONS = {"no_projection": 1, "u1_from_p": 2}


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("ekf_meas") / "libekf_meas_test.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-shared", "-fPIC", "-I", ROOT, "-o", so,
                           os.path.join(ROOT, "tests", "cpp", "ekf_meas_test.cpp")])
    f = C.CDLL(so).ekf_meas_run
    f.argtypes = [C.c_void_p] * 6 + [C.c_int] + [C.c_void_p] * 3
    f.restype = None

    def run(calib, clone, pos, z, gravity, mutate=0):
        T = np.array(calib.T_cam1_cam0, dtype=np.float64).reshape(4, 4)       # CAMState::T_cam0_cam1 (msckf_vio.cpp:121-122)
        R, t = np.ascontiguousarray(T[:3, :3]), np.ascontiguousarray(T[:3, 3])
        a = [np.ascontiguousarray(x, dtype=np.float64) for x in (clone, pos, z, gravity)]
        Hx, Hf, r = np.zeros((4, 6)), np.zeros((4, 3)), np.zeros(4)
        f(R.ctypes.data, t.ctypes.data, a[0].ctypes.data, a[1].ctypes.data, a[2].ctypes.data, a[3].ctypes.data, mutate,
          Hx.ctypes.data, Hf.ctypes.data, r.ctypes.data)
        return Hx, Hf, r
    return run


def _problem_cases(calib):
    """Every observation of make_problem (ten clones, twelve features) for a few seeds."""
    for seed in (0, 1, 2):
        pr = ekf_problems.make_problem(calib, seed=seed, n_clones=10, n_feat=12)
        for j in range(len(pr["positions"])):
            for o in range(pr["obs_start"][j], pr["obs_start"][j + 1]):
                yield "seed%d/f%d/o%d" % (seed, j, o), calib, pr["clones"][pr["obs_clone"][o]], pr["positions"][j], pr["obs_z"][o], pr["gravity"]


def _edge_cases(calib):
    pr = ekf_problems.make_problem(calib, seed=7, n_clones=10, n_feat=12)
    clone, pos, z, g = pr["clones"][3].copy(), pr["positions"][0], pr["obs_z"][0], pr["gravity"]
    same = clone.copy()
    same[7:11], same[11:14] = same[0:4], same[4:7]
    yield "null_equals_state", calib, same, pos, z, g
    # R(q) = I exactly and p, depth exactly representable: p_c0 = (0, 0, 5), the feature on cam0's optical axis
    axis = clone.copy()
    axis[0:4], axis[4:7] = [0.0, 0.0, 0.0, 1.0], [0.25, -0.5, 1.0]
    yield "on_optical_axis", calib, axis, np.array([0.25, -0.5, 6.0]), z, g
    ident = Calib.from_buffer_copy(calib)
    for i in range(3):
        for k in range(3):
            ident.T_cam1_cam0[4 * i + k] = 1.0 if i == k else 0.0
    yield "identity_R_c0_c1", ident, clone, pos, z, g
    for ax in range(3):
        ga = np.zeros(3)
        ga[ax] = 9.81 if ax else -9.81
        yield "gravity_axis%d" % ax, calib, clone, pos, z, ga


def test_device_measurement_jacobian_equals_oracle(oracle, harness):
    """H_x (projected), H_f and r of the device source == the oracle's, as floats (== : the sign of a zero is not compared).
    Measured on the CPU: the largest difference over all inputs is 0 ulp; the bar is exact equality."""
    calib = oracle.euroc_calib(376, 240)
    cfg = default_ekf_cfg(max_cam_state_size=10)
    n = 0
    for name, cal, clone, pos, z, g in list(_problem_cases(calib)) + list(_edge_cases(calib)):
        ref = oracle.measurement_jacobian(cal, cfg, g, clone, pos, z)
        got = harness(cal, clone, pos, z, g)
        for what, a, b in zip(("H_x", "H_f", "r"), got, ref):
            assert np.all(np.isfinite(b)), (name, what)
            assert np.array_equal(a, b), (name, what, "max ulps %g" % (np.abs(a - b) / np.spacing(np.abs(b))).max())
        if name == "on_optical_axis":
            assert got[0][0, 1] != 0 and got[2][0] == z[0] and got[2][1] == z[1]      # p_c0[0] = p_c0[1] = 0 exactly
        n += 1
    assert n > 200


@pytest.mark.parametrize("mutation", sorted(MUTATIONS))
def test_bar_has_teeth(oracle, harness, mutation):
    """The comparison above fails when the projection is dropped and when u1 uses p instead of p_null: on every
    observation of the seeded problems the mutated H_x and H_f differ from the oracle's (r does not depend on either)."""
    calib = oracle.euroc_calib(376, 240)
    cfg = default_ekf_cfg(max_cam_state_size=10)
    for name, cal, clone, pos, z, g in _problem_cases(calib):
        ref = oracle.measurement_jacobian(cal, cfg, g, clone, pos, z)
        bad = harness(cal, clone, pos, z, g, mutate=MUTATIONS[mutation])
        assert not np.array_equal(bad[0], ref[0]), name
        assert not np.array_equal(bad[1], ref[1]), name
        assert np.array_equal(bad[2], ref[2]), name
