"""The conditions that keep the feature-stage edge cases (tests/feature_cases.py) from degenerating, the bars of
tests/test_gpu_feature_edges.py, and the proof that the long-double reference (tests/feature_reference.py) would notice a
subtly wrong kernel: all on the CPU, from the reference's counters and the CPU oracle.

  a. every case reaches what it is named for (valid and invalid triangulations per kernel variant, Huber-weighted
     measurements, rejected Levenberg-Marquardt steps, the size-class boundaries, the slot patterns);
  b. nothing has to be excluded on the device: no |rho| below 1e-6, no gamma within GAMMA_BAR of its threshold;
  c. TRI_BAR and GAMMA_BAR are eight times the largest difference between the double-precision oracle and the long-double
     reference over all cases, re-measured here against the committed constants;
  d. each of feature_reference.MUTATIONS moves its output beyond the corresponding bar.
"""
import functools

import numpy as np
import pytest

import feature_cases as FC
import feature_reference as FR

pytestmark = pytest.mark.skipif(not FR.HAVE_LONG_DOUBLE, reason=FR.NEED_LONG_DOUBLE)

# Measured by test_bars_are_eight_times_the_oracles_own_difference (x86-64, 80-bit long double): the largest
# |d(alpha, beta, rho)| of oracle against reference is 3.85e-9 (pair_w12_65), the largest relative gamma difference 4.54e-13
# (pair_w64_129).  The margin of 8 covers Levenberg-Marquardt paths that part by a rounding at a cost comparison.
TRI_BAR = 3.1e-8          # < 5e-7, the procedure's own stopping step
GAMMA_BAR = 3.7e-12       # relative; <= 1e-7, the bar of test_ekf_update_matches_oracle
RHO_MIN = 1e-6
SIGMA2 = 0.035 ** 2       # default_ekf_cfg().noise_feature ** 2

ALL = sorted(FC.CASES)


@functools.lru_cache(maxsize=None)
def evaluated(name):
    """Oracle and reference over one case: dict(case, tri (reference triangulations), valid (reference), valid_oracle,
    pos_oracle, d_tri (largest |d(alpha, beta, rho)| over the features valid in both), gamma_ref / pass_ref (reference, at
    the reference's positions), d_gamma (largest relative difference oracle against reference at the oracle's positions))."""
    from oracle import oracle_py as O
    O.build()
    chi2 = FR.chi2_table()
    c = FC.case(name)
    n = len(c["cls"])
    tri = FC.reference_triangulation(name)
    idx, starts = FC.init_problem(c)
    pos_o, valid_o = O.triangulate(c["calib"], c["clones"], starts, c["init_clone"], c["init_z"])
    pos = c["positions"].copy()
    pos[idx] = pos_o
    valid_oracle = np.ones(n, bool)
    valid_oracle[idx] = valid_o.astype(bool)
    valid = np.array([True if t is None else t["valid"] for t in tri])
    pos_ref = c["positions"].astype(FR.LD)
    d_tri = 0.0
    for j in idx:
        pos_ref[j] = tri[j]["position"]
        if valid[j] and valid_oracle[j]:
            got = FR.to_inverse_depth(c["clones"], c["init_clone"][c["init_start"][j]], pos[j])
            d_tri = max(d_tri, float(np.abs(got - tri[j]["solution"]).max()))
    keep = np.flatnonzero(valid & valid_oracle)
    orc = FC.oracle_update(O, c, pos, keep)
    g_at_oracle, p_at_oracle = FC.reference_gates(c, pos, SIGMA2, chi2, only=keep)
    ev = orc["gamma"] >= 0                       # (the oracle stops evaluating at the row cap)
    d_gamma = float(np.max(np.abs(g_at_oracle[ev] - orc["gamma"][ev]) / g_at_oracle[ev])) if ev.any() else 0.0
    gamma_ref, pass_ref = FC.reference_gates(c, pos_ref, SIGMA2, chi2, only=np.flatnonzero(valid))
    return dict(case=c, tri=tri, valid=valid, valid_oracle=valid_oracle, pos_oracle=pos, d_tri=d_tri, d_gamma=d_gamma,
                gamma_ref=gamma_ref, pass_ref=pass_ref, pass_at_oracle=p_at_oracle, oracle=orc, evaluated=ev, chi2=chi2)


def _counters(names):
    out = dict(huber=0, rejected=0, outer=0, failed=0)
    for name in names:
        for t in FC.reference_triangulation(name):
            if t is not None:
                for k in out:
                    out[k] += t["counters"][k]
    return out


@pytest.mark.parametrize("name", ALL)
def test_oracle_and_reference_agree_on_validity_and_gate(name):
    e = evaluated(name)
    c = e["case"]
    assert np.array_equal(e["valid"], e["valid_oracle"])
    ev = e["evaluated"]
    assert np.array_equal(e["pass_at_oracle"][ev], e["oracle"]["passed"][ev].astype(bool))
    v = e["valid"]
    print("%s (%s): %d valid, %d invalid, %d pass, %d gated out; counters %s; |d(a,b,rho)| %.2e, gamma %.2e"
          % (name, c["variant"], int(v.sum()), int((~v).sum()), int(e["pass_ref"].sum()), int((v & ~e["pass_ref"]).sum()),
             _counters([name]), e["d_tri"], e["d_gamma"]))


def test_every_kernel_variant_sees_valid_and_invalid_triangulations():
    """At least 5 invalid and 5 valid triangulations (needs_init features) per kernel variant, both passing and gated-out
    features per variant, and in every far set a real mix."""
    count = {}
    for name in ALL:
        e = evaluated(name)
        for j, cls in enumerate(e["case"]["cls"]):
            k = count.setdefault(cls, dict(valid=0, invalid=0, passed=0, gated=0))
            if e["case"]["needs_init"][j]:
                k["valid" if e["valid"][j] else "invalid"] += 1
            if e["valid"][j]:
                k["passed" if e["pass_ref"][j] else "gated"] += 1
    print(count)
    assert sorted(count) == ["big", "pair", "small", "wave"]
    for cls, k in count.items():
        assert min(k.values()) >= 5, (cls, k)
    for name in FC.FAR_SETS:
        e = evaluated(name)
        init = e["case"]["needs_init"].astype(bool)
        assert (e["valid"] & init).sum() >= 5 and (~e["valid"]).sum() >= 3, name
    for name in ("pair_w12_65", "pair_w64_129"):      # the natural mix of the far pair sets, beyond the placed ones
        assert (~evaluated(name)["valid"]).sum() >= 10


def test_far_sets_reach_the_huber_weight_and_rejected_steps():
    for name in FC.FAR_SETS:
        k = _counters([name])
        print(name, k)
        assert k["huber"] >= 10 and k["rejected"] >= 10, (name, k)
    total = _counters(ALL)
    print("all cases:", total)
    assert total["failed"] == 0           # (no case drives the damped 3 x 3 system out of positive definiteness)


def test_class_boundaries_are_present():
    seen = set()
    for name in ALL:
        c = FC.case(name)
        for s, cls in zip(c["specs"], c["cls"]):
            seen.add((cls, len(s["jac"]), len(s["init"]) if s["needs_init"] else 0))
    pair_inits = {k for cls, m, k in seen if cls == "pair"}
    assert {0, 1, 2, 3, 32, 33, 64} <= pair_inits
    for m in (2, 3, 4):
        assert ("wave", m, m) in seen
        assert {k for cls, mm, k in seen if cls == "wave" and mm == m} >= {0, 5, 16, 17, 32}
    assert FC.case("wave_w64_257")["variant"] == "wave" and FC.case("wave_w64_257_leaves")["variant"] == "mixed"
    assert sum(len(s["init"]) == 33 for s in FC.case("wave_w64_257_leaves")["specs"]) == 1
    for key in (("small", 5, 5), ("small", 16, 16), ("small", 5, 16), ("small", 5, 0), ("big", 5, 17)):
        assert key in seen, key
    for m in (17, 30, 31, 32, 33, 63, 64):
        assert ("big", m, m) in seen, m
    # both sides of the 120-row boundary of the gate matrix, in a 32-clone and in a 64-clone window
    for name in ("big_w32", "big_w64"):
        e = evaluated(name)
        for m in (30, 31):
            js = [j for j, s in enumerate(e["case"]["specs"]) if len(s["jac"]) == m]
            assert (4 * m <= FC.GATE_LDS_ROWS) == (m == 30)
            assert any(not e["valid"][j] for j in js), (name, m, "invalid")
            assert any(e["valid"][j] and not e["pass_ref"][j] for j in js), (name, m, "gated out")
            assert any(e["pass_ref"][j] for j in js), (name, m, "pass")


@pytest.mark.parametrize("name", ["slots_small_65", "slots_small_129", "slots_big_65", "slots_big_129"])
def test_slot_patterns(name):
    """Groups 0..3 see [invalid, pass], [pass, invalid], [gated-out, pass], [pass, gated-out]; the 129-feature sets give
    group 0 a third feature; all members are of one class."""
    e = evaluated(name)
    c = e["case"]
    n = len(c["cls"])
    assert len(set(c["cls"])) == 1 and n > FC.EKF_SLOTS

    def kind(j):
        return "invalid" if not e["valid"][j] else ("pass" if e["pass_ref"][j] else "gated")
    assert [kind(0), kind(64)] == ["invalid", "pass"]
    assert [kind(2), kind(66)] == ["gated", "pass"] if n > 66 else kind(2) == "gated"
    if n > 67:
        assert [kind(1), kind(65)] == ["pass", "invalid"]
        assert [kind(3), kind(67)] == ["pass", "gated"]
        assert kind(128) == "pass"
        total = sum(4 * len(s["jac"]) - 3 for j, s in enumerate(c["specs"]) if e["pass_ref"][j])
        assert total > 1500 and c["apply_row_cap"]           # the row cap is hit: the oracle stops, the device does not
        assert (~e["evaluated"][e["valid"]]).any()


def test_nothing_has_to_be_excluded():
    """The GPU tests compare every feature: no |rho| below 1e-6 (the conversion to inverse depth would lose its meaning) and
    no gamma within GAMMA_BAR of its chi-square threshold (the pass bit would be a coin toss)."""
    small_rho, close = [], []
    min_rho, min_margin = np.inf, np.inf
    for name in ALL:
        e = evaluated(name)
        c = e["case"]
        for j, t in enumerate(e["tri"]):
            if t is not None:
                rho = abs(float(t["solution"][2]))
                min_rho = min(min_rho, rho)
                if rho < RHO_MIN:
                    small_rho.append((name, j))
            if e["valid"][j]:
                dof = len(c["specs"][j]["jac"]) + c["dof_offset"]
                margin = abs(float(e["gamma_ref"][j]) / e["chi2"][dof] - 1)
                min_margin = min(min_margin, margin)
                if margin <= GAMMA_BAR:
                    close.append((name, j))
    print("smallest |rho| %.2e, smallest |gamma / chi2 - 1| %.2e" % (min_rho, min_margin))
    assert small_rho == [] and close == []


def test_bars_are_eight_times_the_oracles_own_difference():
    d_tri = max(evaluated(name)["d_tri"] for name in ALL)
    d_gamma = max(evaluated(name)["d_gamma"] for name in ALL)
    print("oracle against long-double reference: |d(alpha, beta, rho)| %.3e -> TRI_BAR %.3e (committed %.3e); "
          "relative gamma %.3e -> GAMMA_BAR %.3e (committed %.3e)" % (d_tri, 8 * d_tri, TRI_BAR, d_gamma, 8 * d_gamma, GAMMA_BAR))
    assert d_tri > 0 and d_gamma > 0
    assert 8 * d_tri <= TRI_BAR <= 8 * d_tri * 1.05           # the committed constants are the measurement, rounded up
    assert 8 * d_gamma <= GAMMA_BAR <= 8 * d_gamma * 1.05
    assert TRI_BAR < 5e-7
    assert GAMMA_BAR <= 1e-7


# ---------------------------------------------------------------------------------------------- d. mutations
def _solution_shift(name, mutate):
    """Largest |d(alpha, beta, rho)| the mutation causes over the features that are valid without it, and how many valid
    bits it flips."""
    c = FC.case(name)
    shift, flips = 0.0, 0
    for j, t in enumerate(FC.reference_triangulation(name)):
        if t is None:
            continue
        m = FR.triangulate(c["calib"], c["clones"], *FC.init_of(c, j), mutate=mutate)
        flips += int(m["valid"] != t["valid"])
        if t["valid"]:
            shift = max(shift, float(np.abs(m["solution"] - t["solution"]).max()))
    return shift, flips


@pytest.mark.parametrize("name", ["pair_w12_65", "wave_w30_65"])
def test_mutation_huber_weight_not_squared(name):
    shift, _ = _solution_shift(name, "huber_not_squared")
    print(name, "shift %.2e" % shift)
    assert shift > 10 * TRI_BAR


def test_mutation_validity_on_cam0_views_only():
    """With cam1 turned by 75 degrees, features on one side lie in front of every cam0 and behind every cam1."""
    e = evaluated("wide_stereo_w12")
    _, flips = _solution_shift("wide_stereo_w12", "valid_cam0_only")
    print("valid bits flipped: %d of %d invalid" % (flips, int((~e["valid"]).sum())))
    assert flips >= 3 and e["valid"].sum() >= 5


@pytest.mark.parametrize("name", ["pair_w12_65", "wave_w12_5", "wide_stereo_w12"])
def test_mutation_cam1_pose_composed_with_T(name):
    shift, _ = _solution_shift(name, "cam1_T_not_inverted")
    print(name, "shift %.2e" % shift)
    assert shift > 10 * TRI_BAR


@pytest.mark.parametrize("mutate", ["no_projection", "no_sigma"])
@pytest.mark.parametrize("name", ["pair_w12_65", "wave_w30_65", "small_w30", "big_w32"])
def test_mutation_moves_gamma(name, mutate):
    e = evaluated(name)
    c = e["case"]
    js = np.flatnonzero(e["valid"])[:8]
    pos = c["positions"].astype(FR.LD)
    for j in js:
        if e["tri"][j] is not None:
            pos[j] = e["tri"][j]["position"]
    g, _ = FC.reference_gates(c, pos, SIGMA2, e["chi2"], only=js, mutate=mutate)
    rel = np.abs(g[js] - e["gamma_ref"][js]) / e["gamma_ref"][js]
    print(name, mutate, "relative gamma shift: min %.2e" % float(rel.min()))
    assert (rel > 10 * GAMMA_BAR).all()


@pytest.mark.parametrize("name", ["pair_w64_129", "wave_w64_257"])
def test_mutation_dof_off_by_one(name):
    e = evaluated(name)
    c = e["case"]
    flips = 0
    for j in np.flatnonzero(e["valid"]):
        flips += int(FR.passes(e["gamma_ref"][j], len(c["specs"][j]["jac"]), c["dof_offset"], e["chi2"], "dof_off_by_one") != e["pass_ref"][j])
    print(name, "pass bits flipped:", flips)
    assert flips >= 1                 # (the device's pass bits are compared exactly: one flipped bit fails the comparison)


def test_reference_update_against_the_oracle():
    """feature_reference.update (no compression, long double) against the oracle's measurementUpdate on a small stack."""
    from oracle import oracle_py as O
    e = evaluated("wave_w12_5")
    c = e["case"]
    keep = np.flatnonzero(e["valid"])
    blocks = []
    for j in keep:
        g = FR.feature_gate(c["calib"], c["clones"], c["P"], e["pos_oracle"][j], *FC.obs_of(c, j), c["gravity"], SIGMA2)
        if FR.passes(g["gamma"], len(c["specs"][j]["jac"]), c["dof_offset"], e["chi2"]):
            blocks.append((g["H_o"], g["r_o"]))
    assert sum(len(b[1]) for b in blocks) == e["oracle"]["rows"] > 0
    dx, P = FR.update(c["P"], blocks, SIGMA2)
    ref = e["oracle"]
    assert np.abs(np.asarray(P, dtype=np.float64) - ref["P"]).max() / np.abs(ref["P"]).max() < 1e-12
    # (the oracle's getter rebuilds the rotational parts of delta_x from quaternion differences, O(|dtheta|^2) accurate)
    assert np.allclose(np.asarray(dx, dtype=np.float64), ref["delta_x"], rtol=1e-5, atol=2e-8)
    assert O is not None
