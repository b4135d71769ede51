"""The filter as a run leaves it: windows that are partly filled, a dead region of the covariance plane that holds old numbers,
and one stream carried through prediction, update and pruning across every size-class limit of the update.

Part 1 (ROOMY): problems of update_cases.CASES on a stream with room for more clones than the problem has.  The plane of such
a stream is ld x ld with ld = align_up(21 + 6 capacity, 8); only [0, d) x [0, d) is live (ekf_device.h).  The dead region is
poisoned through the ABI alone: mskf_ekf_set_cov with EXTRA more clones whose rows and columns carry POISON_SCALE max|P|, then
the trailing clones are removed again.  k_ekf_remove_clone writes P_dst[0:dn, 0:dn] out of place and the two planes are then
swapped, so which plane is current, and what its dead region holds, depends on the number of removals: plane_after() is the
model of that (numpy, no device), and removals() is chosen from it.

    set_cov           : A = P_full (d + 36), B = 0; current A
    removal 1 (two)   : B[0:d+24, 0:d+24] = A; current B, whose dead region is poisoned up to d + 24 only
    removal 2 (two)   : A[0:d+12, 0:d+12] = B (the values it already had); current A: all 36 poisoned rows and columns
    removal 3         : current B again, poisoned up to d + 24: short of "within 32 of the live block"
    removal 4         : current A: poisoned up to d + 36

Three removals of two clones each therefore leave rows d + 24 .. d + 31 of the current plane zero.  An even number of
removals is needed: two clones, two clones, one clone, one clone.

Part 2 (the chain): build_chain lays out one stream's calls from mskf_ekf_reset on; ref_* are the long-double steps from a given
P, double_* their plain numpy double restatement (the proof that the bars can be met, and the carrier of the planted mistakes).
"""
import functools

import numpy as np

import ekf_reference as R
import feature_cases as FC
import feature_reference as FR
import update_cases as U

LD = FR.LD
N = 21
EXTRA = 6                          # clones of poison beyond the problem's window
WIDE = 64                          # second capacity for the windows up to WIDE_UP_TO
WIDE_UP_TO = 31
POISON_SCALE = 1e6
NEAR = 32                          # one GEMM tile: the dead rows and columns a tile of the live block can reach

ROOMY = ["small4_w4_k39_m3", "small4_w30_k598_m1", "gen5_w5_m3", "gen6_w30_m1", "lone97_w16_m3", "scatter_w30_few_m3", "gap_w12_m3",
         "fallback_w15_m0", "chol_w30_m1", "chol_w31_m1", "chol_w31_bias_m0", "trsm_w34_m3", "trsm_w35_m3", "tsqr_w42_k257_m3",
         "tsqr_w43_k273_m3"]
ROOMY_BATCH = ("chol_w30_m1", "tsqr_w43_k273_m3", "gen5_w5_m3")      # two roomy streams of capacity WIDE beside a full one


def capacities(window):
    return [window + EXTRA] + ([WIDE] if window <= WIDE_UP_TO else [])


ROOMY_RUNS = [(name, cap) for name in ROOMY for cap in capacities(U.PROBLEMS[U.CASES[name][0]]["window"])]


def ld_of(capacity):
    return (N + 6 * capacity + 7) // 8 * 8


def poisoned_full(P, seed):
    """P in the leading block of a covariance with EXTRA more clones; the trailing 36 rows and columns hold symmetric values
    of random sign and magnitude POISON_SCALE max|P|."""
    P = np.asarray(P, dtype=np.float64)
    d = len(P)
    rng = np.random.default_rng(seed)
    full = rng.choice([-1.0, 1.0], size=(d + 6 * EXTRA, d + 6 * EXTRA)) * (POISON_SCALE * np.abs(P).max())
    full = np.triu(full) + np.triu(full, 1).T
    full[:d, :d] = P
    return full


def removals(window):
    """Pairs for mskf_ekf_remove_clones_batch that take the EXTRA trailing clones away and leave the plane of set_cov current."""
    W = window
    return [(W + 4, W + 5), (W + 2, W + 3), (W + 1, -1), (W, -1)]


def delete_clones(P, pair):
    drop = set()
    for c in pair:
        if c >= 0:
            drop |= set(range(N + 6 * c, N + 6 * c + 6))
    keep = [i for i in range(P.shape[0]) if i not in drop]
    return P[np.ix_(keep, keep)]


def plane_after(P_full, capacity, pairs, wrong_plane=False):
    """numpy model of mskf_ekf_set_cov(P_full) followed by mskf_ekf_remove_clones_batch for each pair: (current plane ld x ld,
    d).  wrong_plane: the planted mistake of a removal that forgets the swap (the caller goes on reading the old plane)."""
    ld = ld_of(capacity)
    cur, alt = np.zeros((ld, ld)), np.zeros((ld, ld))
    d = len(P_full)
    cur[:d, :d] = P_full
    for pair in pairs:
        new = delete_clones(cur[:d, :d], pair)
        dn = len(new)
        alt[:dn, :dn] = new
        if not wrong_plane:
            cur, alt = alt, cur
        d = dn
    return cur, d


def dead_mask(ld, d):
    m = np.ones((ld, ld), bool)
    m[:d, :d] = False
    return m


def near_dead_is_poisoned(plane, d, P):
    """Every entry of the dead rows and columns within NEAR of the live block is at least 1e5 max|P| in magnitude."""
    hi = min(d + NEAR, plane.shape[0])
    near = np.zeros(plane.shape, bool)
    near[:hi, :hi] = True
    near[:d, :d] = False
    return bool((np.abs(plane[near]) >= 1e5 * np.abs(P).max()).all())


# ---------------------------------------------------------------------------------------------- part 2: the chain
CAPACITY = 45
SIGMA2 = U.SIGMA2
NOISE = 5e-4                       # as update_cases: the gates do not depend on P
FULL_MODE, GRAM_MODE, GRAM_UP_TO = 3, 1, 33
ALL_ACTIVE_AT = (5, 6, 16, 30, 31, 32, 34, 35, 42, 43)          # the limits, in the order the window grows through them
FEW_AT, FEW_ACTIVE, FEW_ROWS = 38, 11, 45                        # the st <= na update: 11 scattered clones, 45 rows for 66 columns
SMALL_ROWS = 39                                                  # 4 active clones, three features of four observations
PRUNE_FEATURES = 40                                              # two observations each: 200 rows on 12 columns
REQUIRED = {"small", "n1=31", "n1=37", "n1=97", "chol_lds@30", "chol@31", "n1=193", "l_fits@34", "direct@35", "tsqr<32,2,2>@42", "tsqr<16,4,2>@43",
            "uncompressed", "pairs", "tsqr<32,2,2>@42 swapped", "tsqr<16,4,2>@43 swapped"}


def all_active_rows(n):
    """The fewest stacked rows above 6 n + 8 that split_rows lays over n clones in features of three and more observations."""
    r = 6 * n + 9
    while True:
        try:
            if min(U.split_rows(r, n)) >= 3:
                return r
        except ValueError:
            pass
        r += 1


def _spread(n, k):
    return tuple(sorted(set(int(round(i * (n - 1) / (k - 1))) for i in range(k))))


def _update_op(index, n, kind, pair=None):
    from oracle import oracle_py as O
    if kind == "all":
        active, rows = tuple(range(n)), all_active_rows(n)
    elif kind == "small":
        active, rows = (tuple(range(n)) if n <= 4 else _spread(n, 4)), (27 if n == 3 else SMALL_ROWS)
    elif kind == "few":
        active, rows = _spread(n, FEW_ACTIVE), FEW_ROWS
    else:
        active, rows = tuple(pair), 5 * PRUNE_FEATURES
    if kind == "pairs":
        specs = [FC.spec(pair, needs_init=0) for _ in range(PRUNE_FEATURES)]
    else:
        specs, off = [], 0
        for k in U.split_rows(rows, len(active)):
            specs.append(FC.spec(sorted(active[(off + i) % len(active)] for i in range(k)), needs_init=0))
            off += k
    c = dict(FC.build_case(O.euroc_calib(376, 240), "chain%d" % index, 9000 + index, n, specs, noise=NOISE, depth_scale=30.0 if kind == "pairs" else 1.0,
                           dof_offset=0 if kind == "pairs" else -1))
    del c["P"]                                                   # the chain's covariance is the stream's own
    na = 6 * len(active)
    c.update(op="update", kind=kind, n=n, d=N + 6 * n, active=sorted(active), na=na, n1=na + 1, st=rows,
             route="small" if na <= U.SU_MAX_NA else "general")
    return c


def _predict_op(index, rng):
    steps = R.imu_steps(3, 0.005, gyro=(0.2, -1.0 + 0.05 * index, 0.5), q0=R.quat_axis_angle((1.0, 2.0, 3.0), 2.0), seed=7000 + index, jitter=0.05)
    return dict(op="predict", steps=steps, J=R.augment_jacobian(rng))


@functools.lru_cache(maxsize=None)
def build_chain(seed=2024):
    """The ops of one stream of capacity 45, from mskf_ekf_reset on: per cycle a prediction with augmentation (n -> n + 1
    clones) and, from three clones on, an update built for the current clone count.  ALL_ACTIVE_AT, FEW_AT and the two
    prunings sit on the limits; between them odd windows take the small route (4 active clones) and even ones are all active.
    At 44 clones: the pruning-shaped update on clones (0, 1), their removal, an all-active update at 42 clones on the swapped
    plane, three more cycles (43, 44, 45 clones), the second pruning at 45, and one more cycle on the plane that now holds
    the 45-clone covariance of before in its dead region.  Returns (P0, ops)."""
    rng = np.random.default_rng(seed)
    P0 = R.spd(N, rng)
    ops = []

    def cycle(n, kind):
        ops.append(_predict_op(len(ops), rng))
        if kind:
            ops.append(_update_op(len(ops), n, kind))

    for n in range(1, 45):
        kind = None if n < 3 else "small" if n <= 4 else "all" if n in ALL_ACTIVE_AT else "few" if n == FEW_AT else "small" if n % 2 else "all"
        cycle(n, kind)
    ops.append(_update_op(len(ops), 44, "pairs", (0, 1)))
    ops.append(dict(op="remove", pair=(0, 1)))
    ops.append(_update_op(len(ops), 42, "all"))
    cycle(43, "all")
    cycle(44, "few")
    cycle(45, "all")
    ops.append(_update_op(len(ops), 45, "pairs", (1, 3)))
    ops.append(dict(op="remove", pair=(1, 3)))
    cycle(44, "all")
    return P0, ops


def chain_ops(mode):
    """The ops the chain runs in `mode`: all of them in mode 3; in mode 1 those up to GRAM_UP_TO clones (the Gram route differs
    from mode 3 in the factorisation classes, and those lie below that count)."""
    P0, ops = build_chain()
    if mode == FULL_MODE:
        return P0, list(ops)
    out, n = [], 0
    for o in ops:
        n += o["op"] == "predict"
        if n > GRAM_UP_TO:
            break
        out.append(o)
    return P0, out


def branches(c, swaps):
    """The names of REQUIRED an update reaches, from its shapes alone."""
    out = set()
    if c["kind"] == "pairs":
        return {"pairs"}
    if c["route"] == "small":
        return {"small"}
    if c["st"] <= c["na"]:
        return {"uncompressed"}
    if c["n1"] in (31, 37, 97, 193):
        out.add("n1=%d" % c["n1"])
    n = c["n"]
    if len(c["active"]) == n:
        if n in (30, 31):
            out.add(("chol_lds@%d" if U.chol_class(n) == 0 else "chol@%d") % n)
        if n in (34, 35):
            out.add(("l_fits@%d" if U.l_fits(c["na"]) else "direct@%d") % n)
        if n in (42, 43):
            out.add(("tsqr<32,2,2>@%d" if U.tsqr_class(n) == 0 else "tsqr<16,4,2>@%d") % n + (" swapped" if swaps % 2 else ""))
    return out


def used_qr(c, mode):
    return U.predicted(c["route"], mode, c["st"], c["na"], False)


# ------------------------------------------------------------------------------- the reference of one step, from a given P
def ref_predict(P, o, qc):
    P1 = R.propagate(P, o["steps"], qc)[0]
    return R.augment(P1, o["J"])


def ref_gates(c, P):
    """Long-double gate of every feature on P -> dict(gamma, passed, margin, H, r)."""
    chi2 = FR.chi2_table()
    nf = len(c["specs"])
    gamma, passed, blocks = np.zeros(nf, dtype=LD), np.zeros(nf, bool), []
    for j in range(nf):
        oc, oz = FC.obs_of(c, j)
        g = FR.feature_gate(c["calib"], c["clones"], P, c["positions"][j], oc, oz, c["gravity"], SIGMA2)
        gamma[j] = np.inf if g["gamma"] is None else g["gamma"]
        passed[j] = FR.passes(g["gamma"], len(oc), c["dof_offset"], chi2)
        if passed[j]:
            blocks.append((g["H_o"], g["r_o"]))
    dof = np.array([len(s["jac"]) + c["dof_offset"] for s in c["specs"]])
    return dict(gamma=gamma, passed=passed, margin=gamma / chi2[dof], H=np.vstack([b[0] for b in blocks]), r=np.concatenate([b[1] for b in blocks]))


def ref_update(c, P, gates, gram):
    """(plain (delta_x, P'), with-prior (delta_x, P') or None) of the update of P, long double."""
    cp = dict(c, P=np.asarray(P))
    plain = U.update_plain(cp, gates["H"], gates["r"])
    return plain, (U.update_with_prior(cp, gates["H"], gates["r"]) if gram else None)


def bias_quantity(c, P, gates):
    cols = U.act_columns(c)
    return float(U.lam_of(c, gates["H"]) * np.diag(np.asarray(P))[cols].max() / (U.QR_BIAS_LIMIT * SIGMA2))


# ------------------------------------------------------------------------------- plain numpy double restatement of the steps
def double_predict(P, o, qc):
    P = np.array(P, dtype=np.float64)
    for st in o["steps"]:
        Phi, Q = (np.asarray(x, dtype=np.float64) for x in R.phi_q(st, qc))
        Pn = P.copy()
        Pn[:N, :N] = Phi @ P[:N, :N] @ Phi.T + Q
        Pn[:N, N:] = Phi @ P[:N, N:]
        Pn[N:, :N] = Pn[:N, N:].T
        Pn[:N, :N] = (Pn[:N, :N] + Pn[:N, :N].T) / 2
        P = Pn
    d, J = len(P), np.asarray(o["J"], dtype=np.float64)
    Pn = np.zeros((d + 6, d + 6))
    Pn[:d, :d] = P
    Pn[d:, :d] = J @ P[:N, :d]
    Pn[:d, d:] = Pn[d:, :d].T
    JJ = J @ P[:N, :N] @ J.T
    Pn[d:, d:] = (JJ + JJ.T) / 2
    return Pn


def double_update(c, P, gates, gram, d=None, stale_T=None):
    """The update in numpy double: Cholesky of S = H P H^T + sigma^2 I for the Householder and uncompressed routes,
    update_cases.gram_double for the Gram route.  d, stale_T: planted mistakes (the live size taken from another cycle; rows of
    a previous, larger update's T left under this one's)."""
    from scipy.linalg import solve_triangular
    P = np.asarray(P, dtype=np.float64)
    if gram:
        return U.gram_double(dict(c, P=P), gates["H"], gates["r"])
    H, r = np.asarray(gates["H"], dtype=np.float64), np.asarray(gates["r"], dtype=np.float64)
    dd = len(P) if d is None else d
    HP = H[:, :dd] @ P[:dd, :]
    if stale_T is not None:
        HP = np.vstack([HP, stale_T])
        H = np.vstack([H, np.zeros((len(stale_T), H.shape[1]))])
        r = np.concatenate([r, np.zeros(len(stale_T))])
    S = HP[:, :dd] @ H[:, :dd].T + SIGMA2 * np.eye(len(H))
    L = np.linalg.cholesky((S + S.T) / 2)
    Y = solve_triangular(L, HP, lower=True)
    Pn = P - Y.T @ Y
    return Y.T @ solve_triangular(L, r, lower=True), (Pn + Pn.T) / 2


def rel(got, ref):
    ref = np.asarray(ref, dtype=LD)
    return float(np.abs(np.asarray(got, dtype=LD) - ref).max() / max(np.abs(ref).max(), LD(1e-300)))


def predict_errors(got, ref, d):
    """Per block (P_II, P_IC, the new clone's rows) max|dP| / max|P| of a predicted (d + 6) x (d + 6) covariance."""
    err = R.block_errors(got[:, :d], ref[:, :d])
    err["new"] = rel(got[d:, :], ref[d:, :])
    return err
