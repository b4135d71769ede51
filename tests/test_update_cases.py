"""The conditions that keep the dense-update edge cases (tests/update_cases.py) on the branch they are named for, the bars of
tests/test_gpu_update_routes.py, and the proof that the long-double reference would notice a subtly wrong kernel: all on the
CPU, from the shapes, the reference's own gate, H and P, and the CPU oracle.  Nothing here reads the device.

  a. shape: every case reaches its row of the table (na, n1, st, K, route, used_qr; chol_class, tsqr_class, l_fits and the
     tsqr_wide room class, worked out from the shapes);
  b. gate: every stacked feature passes with gamma < 0.5 chi2[dof], the placed outlier does not; the bias quantity is >= 10
     where the flag must be raised and <= 0.1 where the Gram factor must stay;
  c. the double-precision oracle stays within one eighth of the Householder bars from the long-double reference on every
     problem (a problem that does not is too ill-conditioned for the bar and gets another seed);
  d. the Gram algebra in plain numpy double stays within one eighth of the Gram bar from update_with_prior, and
     update_with_prior within one eighth of QR_BIAS_LIMIT from the plain reference;
  e. five mutations of the reference's input or output move D_P or D_x beyond 100 times the bar, on every family.
"""
import numpy as np
import pytest

import feature_reference as FR
import update_cases as U

pytestmark = pytest.mark.skipif(not FR.HAVE_LONG_DOUBLE, reason=FR.NEED_LONG_DOUBLE)

# Measured here (x86-64, 80-bit long double) by test_reference_against_the_oracle and test_gram_route_is_feasible_in_double,
# the largest over all problems / Gram cases:
#   oracle against the plain reference        D_P 5.9e-14 (smallbias_w12)    D_x 1.2e-12 (small3_w30)      bars / 8: 1.25e-13, 1.25e-10
#     (D_P 2.6e-15 at most on the problems without an inflated state; without that state 2.5e-14, chol_w31_bias)
#   numpy Gram against update_with_prior      D_P 1.4e-14 (small4_w30_k598)  D_x 6.9e-15 (small4_w64_k143) bar / 8: 1.25e-10
#   update_with_prior against the reference   D_P 2.3e-10 (small4_w64_k143)                                bar / 8: 1.25e-7
ORACLE_P_MAX, ORACLE_X_MAX = U.HH_P_BAR / 8, U.HH_X_BAR / 8
GRAM_MAX, PRIOR_MAX = U.GRAM_BAR / 8, U.GRAM_PLAIN_BAR / 8

ALL = sorted(U.CASES)
PROBLEMS = sorted(U.PROBLEMS)
GRAM = [n for n in ALL if U.PROBLEMS[U.CASES[n][0]]["modes"][U.CASES[n][1]] == 0]


def _family(name):
    return [U.case(n) for n in ALL if U.case(n)["family"] == name]


# ---------------------------------------------------------------------------------------------- a. shape
@pytest.mark.parametrize("name", ALL)
def test_case_reaches_its_route(name):
    """na, n1, st, K from the reference's gate; route from the clones the features touch (plan_stream); used_qr from the
    shapes and the bias quantity of the reference's H and the case's P."""
    c = U.case(name)
    s = U.stack(c["problem"])
    assert np.array_equal(s["passed"], c["stacked"])
    touched = sorted(set(int(k) for sp in c["specs"] for k in sp["jac"]))
    active = sorted(set(int(k) for j, sp in enumerate(c["specs"]) if s["passed"][j] for k in sp["jac"]))
    assert active == c["active"] and c["na"] == 6 * len(active) and c["n1"] == c["na"] + 1 and c["d"] == 21 + 6 * c["window"]
    ends = np.cumsum(c["rows_of"])
    assert c["st"] == int(c["rows_of"][s["passed"]].sum()) == s["H"].shape[0] <= 650
    assert c["K"] == int(ends[np.flatnonzero(s["passed"])[-1]]) >= c["st"]
    assert c["route"] == ("small" if 6 * len(touched) <= U.SU_MAX_NA else "general")
    assert stream_is_not_a_pair_stack(c)
    q = U.bias_quantity(c["problem"])
    assert (q >= 10.0) if c["bias"] == "forced" else (q <= 0.1), q
    assert c["used_qr"] == U.predicted(c["route"], c["mode"], c["st"], c["na"], q > 1.0)
    assert c["gram"] == (c["used_qr"] == 0)
    if c["gram"]:
        assert c["st"] > c["na"]                         # (G would be singular by construction otherwise)
    print("%s: window %d, na %d, st %d, K %d, mode %d, %s route, used_qr %d, bias quantity %.2e: %s"
          % (name, c["window"], c["na"], c["st"], c["K"], c["mode"], c["route"], c["used_qr"], q, c["limit"]))


def stream_is_not_a_pair_stack(c):
    return not all(len(sp["jac"]) == 2 for sp in c["specs"])


def test_small_route_rows():
    """Three clones: np = 190 pairs, one group, one slot per thread.  Four clones: np = 325, the second slot; K below one
    128-row chunk, K in (512, 640) (five blocks over four wavefronts: 2, 1, 1, 1, the fifth partial), d = 405 beyond one pass of
    256 threads, and st <= na in mode 3, which the fused kernel compresses with its TSQR (used_qr 1, not 2)."""
    for c in _family("small3"):
        n_pairs = c["n1"] * (c["n1"] + 1) // 2
        assert c["na"] == 18 and 128 < n_pairs == 190 <= 256 and all(len(sp["jac"]) == 3 for sp in c["specs"])
    assert sorted((c["window"], c["mode"]) for c in _family("small3")) == [(4, 1), (4, 2), (30, 1), (30, 2)]
    four = _family("small4")
    for c in four:
        assert c["na"] == 24 == U.SU_MAX_NA and c["n1"] * (c["n1"] + 1) // 2 == 325 > 256
    assert {(c["window"], c["mode"]) for c in four} >= {(w, m) for w in (4, 30, 64) for m in (1, 2, 3)}
    assert any(c["K"] < U.SU_CH for c in four)
    assert any(4 * U.SU_CH < c["K"] < 5 * U.SU_CH and c["K"] % U.SU_CH for c in four)
    assert any(c["d"] == 405 > 256 for c in four)
    assert [c["active"] for c in four if c["window"] == 30][0] == [26, 27, 28, 29]
    few = [c for c in four if c["st"] <= c["na"]]
    assert few and all(c["mode"] == 3 and c["used_qr"] == 1 for c in few)
    (b,) = _family("smallbias")
    assert b["window"] == 12 and b["na"] == 24 and b["mode"] == 0 and b["used_qr"] == 1 and b["st"] > b["na"]


def test_general_route_rows():
    """The first general sizes, the lone residual tile, the scattered active set and the gated gap."""
    first = _family("first_general")
    assert {(c["window"], c["n1"], c["mode"]) for c in first} == {(5, 31, 1), (5, 31, 3), (30, 31, 1), (30, 31, 3), (30, 37, 1), (30, 37, 3)}
    for c in first:
        assert c["na"] == U.SU_MAX_NA + 6 * (1 if c["n1"] == 31 else 2)
        assert -(-c["n1"] // U.GEMM_TILE) == (1 if c["n1"] == 31 else 2) and c["na"] < c["st"] and c["K"] < 128
    lone = _family("lone_residual")
    assert sorted(c["mode"] for c in lone) == [1, 3]
    for c in lone:
        assert c["n1"] == 97 and c["n1"] % U.GEMM_TILE == 1 and c["n1"] % U.LNB == 1 and c["na"] % 32 == 0 and U.chol_class(c["window"]) == 0
    sc = _family("scatter")
    assert sorted((c["mode"], c["used_qr"]) for c in sc) == [(0, 2), (1, 0), (3, 1), (3, 2)]
    for c in sc:
        assert c["window"] == 30 and len(c["active"]) == 11 and c["active"] != list(range(11)) and (c["used_qr"] == 2) == (c["st"] <= c["na"])
        assert any(b - a > 1 for a, b in zip(c["active"], c["active"][1:])) and 0 in c["active"] and 29 in c["active"]
    gap = _family("gated_gap")
    assert sorted(c["mode"] for c in gap) == [1, 3]
    for c in gap:
        (g,) = c["gated"]
        assert 0 < g < len(c["specs"]) - 1 and c["K"] == c["st"] + c["rows_of"][g] and c["st"] > c["na"] == 72


def test_fallback_and_factorisation_rows():
    """The three tsqr_wide instantiations by the room class (3072 doubles against 48 n1 and 32 n1), the two factorisation
    kernels at nt = 181 / 187 with which = 0 (modes 1, 0) and which = 1 (all modes), the global kernel with a last panel of one row
    and at the largest window."""
    fb = {c["window"]: c for c in _family("fallback")}
    assert sorted(fb) == [10, 15, 30]
    for w, n1, rl in ((10, 61, 12), (15, 91, 8), (30, 181, 4)):
        c = fb[w]
        nt = 6 * w + 1
        room = nt * (nt + 1) // 2 + U.CHOL_PAN_RS * U.LNB - c["n1"] * (c["n1"] + 1) // 2
        assert c["n1"] == n1 and room == 3072 and U.chol_class(w) == 0 and c["mode"] == 0 and c["used_qr"] == 1
        assert U.wide_rows_per_lane(w, n1) == rl == (12 if room >= 48 * n1 else 8 if room >= 32 * n1 else 4)
        assert c["K"] > 4 * rl                                   # more than one row block
    edge = _family("chol_edge")
    assert sorted((c["window"], c["mode"], c["used_qr"]) for c in edge) == [(30, 1, 0), (30, 3, 1), (31, 0, 1), (31, 1, 0), (31, 3, 1)]
    for c in edge:
        assert c["n1"] == 6 * c["window"] + 1 == (181 if c["window"] == 30 else 187)
        assert U.chol_class(c["window"]) == (0 if c["window"] == 30 else 1)
        if c["mode"] == 0:
            assert U.wide_rows_per_lane(31, 187) == 4 and U.LNB * 192 >= 16 * 187        # R in the W buffer, the block in the panel's LDS
    assert U.CHOL_LDS_MAX_ROWS == 181
    (g,) = _family("lone_residual_global")
    assert g["n1"] == 193 and g["n1"] % U.LNB == 1 and g["n1"] % U.GEMM_TILE == 1 and U.chol_class(32) == 1 and g["mode"] == 1
    (b,) = _family("largest_gram")
    assert b["window"] == 64 and b["n1"] == 385 and b["mode"] == 1 and 400 <= b["st"] <= 650 and U.chol_class(64) == 1


def test_solve_and_tsqr_rows():
    """k_ekf_trsm with the register prefetch (n = 204) and with direct staging (n = 210; n = st = 209 uncompressed);
    k_ekf_tsqr<32,2,2> (128-row blocks) at K = 128, 129, 257 and <16,4,2> (64-row blocks) at K = 64, 65, 129."""
    assert U.l_fits(208) and not U.l_fits(209)
    tr = _family("trsm_edge")
    assert sorted((c["window"], c["mode"], c["used_qr"]) for c in tr) == [(34, 1, 0), (34, 3, 1), (35, 1, 0), (35, 3, 1), (35, 3, 2)]
    for c in tr:
        nk = c["st"] if c["used_qr"] == 2 else c["na"]
        assert nk == {(34, 0): 204, (34, 1): 204, (35, 0): 210, (35, 1): 210, (35, 2): 209}[(c["window"], c["used_qr"])]
        assert U.l_fits(nk) == (c["window"] == 34)
    tq = _family("tsqr_edge")
    assert all(c["used_qr"] == 1 and c["mode"] in (2, 3) for c in tq)
    assert U.tsqr_class(42) == 0 and U.tsqr_class(43) == 1 and 6 * 42 + 1 == 253 <= 256 < 259 == 6 * 43 + 1
    assert sorted(c["K"] for c in tq if c["window"] == 42) == [128, 129, 257]
    assert sorted(c["K"] for c in tq if c["window"] == 43) == [64, 65, 129, 273]
    assert any(c["n1"] == 253 and c["mode"] == 3 and c["st"] > c["na"] for c in tq) and any(c["n1"] == 259 and c["mode"] == 3 and c["st"] > c["na"] for c in tq)
    for c in tq:
        assert c["mode"] == (3 if c["st"] > c["na"] else 2)      # mode 3 would leave st <= na uncompressed


# ---------------------------------------------------------------------------------------------- b. gate
@pytest.mark.parametrize("pname", PROBLEMS)
def test_gate_margins(pname):
    c, s = U.problem(pname), U.stack(pname)
    assert float(s["margin"][c["stacked"]].max()) < 0.5
    for g in c["gated"]:
        assert s["margin"][g] > 2.0 and not s["passed"][g]
    assert np.abs(s["r"]).max() > 1e-5                           # (a residual the mutations can take away)


# ---------------------------------------------------------------------------------------------- c. reference against the oracle
@pytest.mark.parametrize("pname", PROBLEMS)
def test_reference_against_the_oracle(oracle, pname):
    c, s = U.problem(pname), U.stack(pname)
    orc = U.oracle_update(oracle, c)
    assert orc["rows"] == c["st"] and np.array_equal(orc["passed"].astype(bool), s["passed"])
    D_P, D_x = U.distances(orc["delta_x"], orc["P"], U.reference(pname))
    print("%s: oracle against long-double reference: D_P %.2e (bar / 8 %.2e), D_x %.2e (bar / 8 %.2e)" % (pname, D_P, ORACLE_P_MAX, D_x, ORACLE_X_MAX))
    assert D_P <= ORACLE_P_MAX and D_x <= ORACLE_X_MAX
    if c["inflated"] is not None:
        B_P, B_x = U.distances(orc["delta_x"], orc["P"], U.reference(pname), exclude=c["inflated"])
        print("%s: without state %d: D_P %.2e, D_x %.2e" % (pname, c["inflated"], B_P, B_x))
        assert B_P <= ORACLE_P_MAX and B_x <= ORACLE_X_MAX


# ---------------------------------------------------------------------------------------------- d. Gram feasibility
@pytest.mark.parametrize("name", GRAM)
def test_gram_route_is_feasible_in_double(name):
    c = U.case(name)
    s = U.stack(c["problem"])
    dx, Pn = U.gram_double(c, s["H"], s["r"])
    prior = U.reference_with_prior(c["problem"])
    D_P, D_x = U.distances(dx, Pn, prior)
    P_P, _ = U.distances(prior[0], prior[1], U.reference(c["problem"]))
    print("%s: numpy Gram against update_with_prior: D_P %.2e, D_x %.2e (bar / 8 %.2e); update_with_prior against the plain reference: D_P %.2e "
          "(bar / 8 %.2e)" % (name, D_P, D_x, GRAM_MAX, P_P, PRIOR_MAX))
    assert D_P <= GRAM_MAX and D_x <= GRAM_MAX and P_P <= PRIOR_MAX


# ---------------------------------------------------------------------------------------------- e. mutations
# one case per family, the smallest
REPRESENTATIVE = {"small3": "small3_w4_m1", "small4": "small4_w4_k39_m3", "smallbias": "smallbias_w12_m0", "first_general": "gen6_w30_m1",
                  "lone_residual": "lone97_w16_m3", "scatter": "scatter_w30_m1", "gated_gap": "gap_w12_m3", "fallback": "fallback_w10_m0",
                  "chol_edge": "chol_w31_m1", "lone_residual_global": "lone193_w32_m1", "trsm_edge": "trsm_w35_few_m3",
                  "tsqr_edge": "tsqr_w43_k129_m2", "largest_gram": "big_w64_m1"}


def _moved(c, mutated, ref):
    """Does the mutated result lie beyond 100 times the case's bar from the reference the case is judged by?"""
    D_P, D_x = U.distances(mutated[0], mutated[1], ref)
    far = D_P > 100 * (U.GRAM_BAR if c["gram"] else U.HH_P_BAR) or D_x > 100 * (U.GRAM_BAR if c["gram"] else U.HH_X_BAR)
    if c["inflated"] is not None:
        B_P, B_x = U.distances(mutated[0], mutated[1], ref, exclude=c["inflated"])
        far = far and (B_P > 100 * U.HH_P_BAR or B_x > 100 * U.HH_X_BAR)
    return far, D_P, D_x


def test_every_family_has_a_representative():
    assert sorted(REPRESENTATIVE) == U.FAMILIES
    for fam, name in REPRESENTATIVE.items():
        assert U.case(name)["family"] == fam


@pytest.mark.parametrize("family", sorted(REPRESENTATIVE))
def test_mutations_move_the_result_beyond_100_bars(family):
    c = U.case(REPRESENTATIVE[family])
    s = U.stack(c["problem"])
    H, r = s["H"], s["r"]
    cols = U.act_columns(c)
    upd = U.update_with_prior if c["gram"] else U.update_plain
    ref = U.reference_with_prior(c["problem"]) if c["gram"] else U.reference(c["problem"])
    muts = {}
    Hm = H.copy(); Hm[:, cols[-1]] = 0
    muts["last active column of H zeroed"] = upd(c, Hm, r)
    muts["last stacked row dropped"] = upd(c, H[:-1], r[:-1])
    rm = r.copy(); rm[-1] = 0
    muts["residual of the last stacked row zeroed"] = upd(c, H, rm)
    for k in (32, 96):
        if k < len(cols):
            i = int(np.argmax(np.abs(H[:, cols[k]])))
            Hm = H.copy(); Hm[i, cols[k]] = 0
            muts["H(%d, compact column %d) zeroed" % (i, k)] = upd(c, Hm, r)
    inactive = [k for k in range(c["window"]) if k not in c["active"]]
    if inactive:
        rows = 21 + 6 * inactive[len(inactive) // 2] + np.arange(6)
        Pm = ref[1].copy()
        Pm[rows, :] = np.asarray(c["P"], dtype=U.LD)[rows, :]
        muts["rows of inactive clone %d of P' left at their prior values" % inactive[len(inactive) // 2]] = (ref[0], Pm)
    assert len(muts) >= 3
    for what, m in muts.items():
        far, D_P, D_x = _moved(c, m, ref)
        print("%s: %s: D_P %.2e, D_x %.2e" % (c["name"], what, D_P, D_x))
        assert far, what
    assert not _moved(c, ref, ref)[0]


def test_mutations_cover_every_kind():
    """Compact columns 32 and 96 and an inactive clone exist among the representatives."""
    cs = [U.case(n) for n in REPRESENTATIVE.values()]
    assert any(32 < c["na"] <= 96 for c in cs) and any(c["na"] > 96 for c in cs) and any(len(c["active"]) < c["window"] for c in cs)
