"""CPU proof of tests/chain_cases.py (no GPU): the poisoning recipe leaves what tests/test_gpu_filter_chain.py asserts before
its updates, the chain reaches every limit it is built for, its gates and its bias quantity keep their margins, a plain numpy
double restatement of every step stays within one eighth of every bar the device is held to (so the bars can be met), and
four planted mistakes move a result at least 100 times beyond its bar.
"""
import time

import numpy as np
import pytest

from msckf_stereo_c_amd.ctypes_types import default_ekf_cfg

import chain_cases as CC
import ekf_reference as R
import feature_reference as FR
import update_cases as U

pytestmark = pytest.mark.skipif(not FR.HAVE_LONG_DOUBLE, reason=FR.NEED_LONG_DOUBLE)

PREDICT_BAR = 1e-12               # tests/test_gpu_filter_predict.py, per block
CPU_BUDGET = 20.0                 # seconds of this thread's CPU time per test (the long-double arithmetic is single-threaded)


def _qc():
    return R.qc_of(default_ekf_cfg())


# ---------------------------------------------------------------------------------------------- part 1: the poisoned window
def test_roomy_cases_exist_and_cover_the_families():
    assert set(CC.ROOMY) <= set(U.CASES)
    assert {U.case(n)["route"] for n in CC.ROOMY} == {"small", "general"}
    assert {U.case(n)["used_qr"] for n in CC.ROOMY} == {0, 1, 2}
    gen = [U.case(n) for n in CC.ROOMY if U.case(n)["route"] == "general"]
    assert {U.chol_class(c["window"]) for c in gen} == {0, 1} and {U.tsqr_class(c["window"]) for c in gen} == {0, 1}
    assert {U.l_fits(c["na"]) for c in gen} == {True, False}
    assert (("chol_w30_m1", 36) in CC.ROOMY_RUNS and ("chol_w30_m1", 64) in CC.ROOMY_RUNS and ("trsm_w34_m3", 40) in CC.ROOMY_RUNS
            and ("trsm_w34_m3", 64) not in CC.ROOMY_RUNS)
    for name, cap in CC.ROOMY_RUNS:
        c = U.case(name)
        assert CC.ld_of(cap) >= c["d"] + 6 * CC.EXTRA >= c["d"] + CC.NEAR           # d well below ld: a whole tile of dead columns


@pytest.mark.parametrize("name,capacity", [("small4_w4_k39_m3", 10), ("chol_w31_m1", 37), ("chol_w30_m1", 64)])
def test_four_removals_leave_the_poisoned_plane_current(name, capacity):
    """plane_after, the numpy model of k_ekf_remove_clone's out-of-place write and the swap: with removals() the live block is
    the case's P bit for bit and every dead row and column within 32 of it is poisoned; with three removals of two clones
    each (the current plane is then the other one) rows d + 24 .. d + 31 are zero."""
    c = U.case(name)
    full = CC.poisoned_full(c["P"], 1)
    assert np.array_equal(full, full.T) and np.array_equal(full[:c["d"], :c["d"]], c["P"])
    assert (np.abs(full[c["d"]:, :]) == CC.POISON_SCALE * np.abs(c["P"]).max()).all()
    plane, d = CC.plane_after(full, capacity, CC.removals(c["window"]))
    assert d == c["d"] and np.array_equal(plane[:d, :d], c["P"])
    assert CC.near_dead_is_poisoned(plane, d, c["P"])
    W = c["window"]
    plane3, d3 = CC.plane_after(full, capacity, [(W + 4, W + 5), (W + 2, W + 3), (W, W + 1)])
    assert d3 == d and np.array_equal(plane3[:d, :d], c["P"])
    assert not CC.near_dead_is_poisoned(plane3, d, c["P"]) and not plane3[d + 24:d + 32, :].any()


def test_double_restatement_meets_the_bars_on_the_roomy_cases():
    """double_update (numpy double) against the long-double references of update_cases, on every case of ROOMY: within one
    eighth of each bar."""
    t0 = time.thread_time()
    for name in CC.ROOMY:
        c = U.case(name)
        s = U.stack(c["problem"])
        dx, Pn = CC.double_update(c, c["P"], s, c["gram"])
        D_P, D_x = U.distances(dx, Pn, U.reference(c["problem"]))
        if c["gram"]:
            G_P, G_x = U.distances(dx, Pn, U.reference_with_prior(c["problem"]))
            assert G_P < U.GRAM_BAR / 8 and G_x < U.GRAM_BAR / 8 and D_P < U.GRAM_PLAIN_BAR / 8, (name, G_P, G_x, D_P)
        elif c["inflated"] is None:
            assert D_P < U.HH_P_BAR / 8 and D_x < U.HH_X_BAR / 8, (name, D_P, D_x)
        else:
            B_P, B_x = U.distances(dx, Pn, U.reference(c["problem"]), exclude=c["inflated"])
            assert max(D_P, B_P) < U.HH_P_BAR / 8 and max(D_x, B_x) < U.HH_X_BAR / 8, (name, D_P, D_x, B_P, B_x)
    assert time.thread_time() - t0 < CPU_BUDGET


# ---------------------------------------------------------------------------------------------- part 2: the chain
def test_chain_reaches_every_limit_in_order():
    """The branches of every update of the chain, re-derived from its shapes (U.predicted, chol_class, tsqr_class, l_fits, the
    route from na): the set equals REQUIRED, the limits come in the order the window grows through them, the window never exceeds the
    capacity, and the mode-1 chain ends at 33 clones with both factorisation classes behind it."""
    P0, ops = CC.chain_ops(CC.FULL_MODE)
    assert P0.shape == (21, 21)
    n, swaps, seen, order = 0, 0, set(), []
    for o in ops:
        if o["op"] == "predict":
            n += 1
        elif o["op"] == "remove":
            assert len(set(o["pair"])) == 2 and max(o["pair"]) < n
            n -= 2
            swaps += 1
        else:
            assert o["n"] == n and o["d"] == 21 + 6 * n and max(o["active"]) < n and o["na"] == 6 * len(o["active"])
            assert o["route"] == ("small" if o["na"] <= U.SU_MAX_NA else "general")
            assert o["st"] == int(sum(4 * len(s["jac"]) - 3 for s in o["specs"]))
            b = CC.branches(o, swaps)
            order += sorted(b - seen)
            seen |= b
            want = 1 if o["route"] == "small" or o["st"] > o["na"] else 2
            assert CC.used_qr(o, CC.FULL_MODE) == want
            if o["kind"] == "pairs":
                assert all(len(s["jac"]) == 2 for s in o["specs"]) and o["dof_offset"] == 0 and not o["apply_row_cap"]
            if o["kind"] == "small":
                assert len(o["active"]) <= 4
        assert n <= CC.CAPACITY
    assert seen == CC.REQUIRED
    want_order = ["small", "n1=31", "n1=37", "n1=97", "chol_lds@30", "chol@31", "n1=193", "l_fits@34", "direct@35", "uncompressed",
                  "tsqr<32,2,2>@42", "tsqr<16,4,2>@43", "pairs", "tsqr<32,2,2>@42 swapped", "tsqr<16,4,2>@43 swapped"]
    assert order == want_order
    assert swaps == 2 and n == 44
    _, gram_ops = CC.chain_ops(CC.GRAM_MODE)
    ups = [o for o in gram_ops if o["op"] == "update"]
    assert max(o["n"] for o in ups) == CC.GRAM_UP_TO and not any(o["op"] == "remove" for o in gram_ops)
    assert {U.chol_class(o["n"]) for o in ups if o["kind"] == "all"} == {0, 1}
    assert all(CC.used_qr(o, CC.GRAM_MODE) == 0 for o in ups)


def _carry(mode, check):
    """Runs the chain twice on the CPU: a long-double chain that carries its own P (margins), and the numpy double restatement
    re-seeded as the device test re-seeds (each step's long-double reference starts from the restatement's own previous P).
    check(kind, figures) is called per step."""
    P0, ops = CC.chain_ops(mode)
    qc = _qc()
    P_ld = np.asarray(P0, dtype=CC.LD)
    P_db = P0.copy()
    for o in ops:
        if o["op"] == "predict":
            d = len(P_db)
            ref = CC.ref_predict(P_db, o, qc)
            P_db = CC.double_predict(P_db, o, qc)
            check("predict", o, CC.predict_errors(P_db, ref, d))
            P_ld = CC.ref_predict(P_ld, o, qc)
        elif o["op"] == "remove":
            P_db, P_ld = CC.delete_clones(P_db, o["pair"]), CC.delete_clones(P_ld, o["pair"])
        else:
            gram = CC.used_qr(o, mode) == 0
            g_ld = CC.ref_gates(o, P_ld)
            check("margins", o, dict(margin=float(g_ld["margin"].max()), passed=bool(g_ld["passed"].all()), bias=CC.bias_quantity(o, P_ld, g_ld)))
            P_ld = CC.ref_update(o, P_ld, g_ld, False)[0][1]
            g = CC.ref_gates(o, P_db)
            plain, prior = CC.ref_update(o, P_db, g, gram)
            dx, Pn = CC.double_update(o, P_db, g, gram)
            fig = dict(zip(("D_P", "D_x"), U.distances(dx, Pn, plain)))
            if gram:
                fig.update(zip(("G_P", "G_x"), U.distances(dx, Pn, prior)))
            fig["min_eig"] = float(np.linalg.eigvalsh(Pn).min()) / float(np.abs(P_db).max())
            check("update_gram" if gram else "update", o, fig)
            P_db = Pn
    return P_ld, P_db


@pytest.mark.parametrize("mode", [CC.FULL_MODE, CC.GRAM_MODE])
def test_chain_margins_hold_and_the_bars_can_be_met(mode):
    """On the self-carried long-double chain every planted-good feature passes its gate with gamma / chi2 <= 0.5 and the bias
    quantity stays below 0.5 (the recorded side of 1, a factor of 2 to spare).  The re-seeded double restatement of every
    prediction, update and removal stays within one eighth of the bar the device test applies to that step."""
    t0 = time.thread_time()
    worst = {}

    def check(kind, o, f):
        for k, v in f.items():
            if not isinstance(v, bool):
                worst[(kind, k)] = max(worst.get((kind, k), -np.inf), v) if k != "min_eig" else min(worst.get((kind, k), np.inf), v)
        if kind == "predict":
            assert all(e <= PREDICT_BAR / 8 for e in f.values()), f
        elif kind == "margins":
            assert f["passed"] and f["margin"] <= 0.5 and f["bias"] <= 0.5, (o["n"], o["kind"], f)
        elif kind == "update":
            assert f["D_P"] < U.HH_P_BAR / 8 and f["D_x"] < U.HH_X_BAR / 8 and f["min_eig"] >= -U.HH_P_BAR / 8, (o["n"], o["kind"], f)
        else:
            assert f["G_P"] < U.GRAM_BAR / 8 and f["G_x"] < U.GRAM_BAR / 8 and f["D_P"] < U.GRAM_PLAIN_BAR / 8 and f["min_eig"] >= -U.GRAM_BAR / 8, (o["n"], f)

    P_ld, P_db = _carry(mode, check)
    print("mode %d: %s; drift of the re-seeded double chain from the self-carried long-double chain %.3e" % (
        mode, ", ".join("%s %s %.2e" % (k[0], k[1], v) for k, v in sorted(worst.items())), CC.rel(P_db, P_ld)))
    assert time.thread_time() - t0 < CPU_BUDGET


# ---------------------------------------------------------------------------------------------- planted mistakes
@pytest.fixture(scope="module")
def mid_chain():
    """The chain in double up to its all-active update at 16 clones: (P before that update, the op, its gates, the plain
    long-double reference, the previous all-active update's T = H P rows)."""
    P0, ops = CC.chain_ops(CC.FULL_MODE)
    qc = _qc()
    P, T_prev = P0.copy(), None
    for o in ops:
        if o["op"] == "predict":
            P = CC.double_predict(P, o, qc)
            continue
        g = CC.ref_gates(o, P)
        if o["n"] == 16:
            return P, o, g, CC.ref_update(o, P, g, False)[0], T_prev
        if o["kind"] == "all":
            T_prev = np.asarray(g["H"], dtype=np.float64) @ P
        P = CC.double_update(o, P, g, False)[1]


def test_planted_mistakes_show_at_100_times_the_bar(mid_chain):
    """Against the long-double reference of the 16-clone update: (a) one dead row of magnitude 1e6 max|P| read as live by
    the product T = H P, (b) the update run with the previous cycle's d, (c) a row of the previous update's T left under
    this one's.  Each moves P' at least 100 times beyond HH_P_BAR; the restatement without them sits within an eighth of it."""
    P, o, g, ref, T_prev = mid_chain
    d = o["d"]
    clean = U.distances(*CC.double_update(o, P, g, False), ref)
    assert clean[0] < U.HH_P_BAR / 8
    # (a) the contraction of T = H P runs one index too far: column d of the stacked rows holds what a wider update left
    # there (here: a copy of the last live column), row d of the plane holds poison
    rng = np.random.default_rng(3)
    poison = rng.choice([-1.0, 1.0], d) * CC.POISON_SCALE * np.abs(P).max()
    H, r = np.asarray(g["H"], dtype=np.float64), np.asarray(g["r"], dtype=np.float64)
    T = H @ P + np.outer(H[:, d - 1], poison)
    S = T @ H.T + CC.SIGMA2 * np.eye(len(H))
    Pn = P - T.T @ np.linalg.solve(S, T)
    assert U.distances(T.T @ np.linalg.solve(S, r), Pn, ref)[0] > 100 * U.HH_P_BAR
    # (b) d of the cycle before
    dx, Pn = CC.double_update(o, P, g, False, d=d - 6)
    assert U.distances(dx, Pn, ref)[0] > 100 * U.HH_P_BAR
    # (c) a stale row of T
    stale = np.zeros((1, d))
    stale[0, :T_prev.shape[1]] = T_prev[-1]
    dx, Pn = CC.double_update(o, P, g, False, stale_T=stale)
    assert U.distances(dx, Pn, ref)[0] > 100 * U.HH_P_BAR


def test_removal_from_the_wrong_plane_shows(mid_chain):
    """The chain's first pruning removes clones 0 and 1.  A caller that goes on reading the plane the removal read from sees
    the old leading block: it differs from the numpy deletion by far more than 100 times any bar, relative to max|P|."""
    P = mid_chain[0]
    full = np.zeros((CC.ld_of(CC.CAPACITY),) * 2)
    full[:len(P), :len(P)] = P
    right, d = CC.plane_after(P, CC.CAPACITY, [(0, 1)])
    wrong, d2 = CC.plane_after(P, CC.CAPACITY, [(0, 1)], wrong_plane=True)
    assert d == d2 == len(P) - 12
    assert np.array_equal(right[:d, :d], CC.delete_clones(P, (0, 1)))
    assert CC.rel(wrong[:d, :d], right[:d, :d]) > 100 * U.GRAM_PLAIN_BAR
