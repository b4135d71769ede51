"""Seeded update problems that drive the DENSE half of the measurement update (k_ekf_gemm<GRAM|T|S2|PUPD>, k_ekf_chol_lds,
k_ekf_chol, k_ekf_tsqr<32,2,2> / <16,4,2>, k_ekf_trsm, k_ekf_small_update and the in-kernel Householder fallback tsqr_wide of
ekf_compress_exit) at every size limit the code branches on, and their long-double reference.

A PROBLEM is a window, a hand-chosen active clone set and a stacked row count: feature_cases.build_case with the positions
given (needs_init = 0), every feature observed by a run of the active set (cyclic, so that the runs cover it), 4 n_obs - 3
rows per feature.  One `outlier` spec in the middle of a stack leaves rows with a zero rowmask inside K.  A CASE is a
problem and a compression_mode; cases of one problem share its reference.

A case records window (d = 21 + 6 window), active / na / n1, st (stacked rows), K (end of the last stacked block), mode,
route ("small" | "general"), used_qr (0 Gram factor, 1 Householder, 2 uncompressed), gram (judged against
update_with_prior), bias ("forced" | "low"), inflated (see FORCED below), family and limit (which kernel limit it sits on).  The expected values
are written down by hand in the table below; tests/test_update_cases.py re-derives every one of them from the shapes and
from the reference's own gate, H and P (never from the device).

The reference: feature_reference.feature_gate per passing feature -> (H_o, r_o), then feature_reference.update, all long
double, no compression (the left null-space basis and the compression change nothing in exact arithmetic).  For the cases
that must stay on the Gram factor, update_with_prior is the same update with na extra rows sqrt(lambda) e_act(i) and zero
residual, lambda = 1e-14 d max diag(H_act^T H_act) from the reference's own H: the operation the kernels define
(G + lambda I), stated exactly.

Where the planned table of cases could not be met literally: a stack of K rows touches at most about K / 2.5 clones, and
compression_mode 3 compresses nothing when st <= na.  The k_ekf_tsqr cases whose K lies below na (K = 128, 129 at 42
clones; 64, 65, 129 at 43) therefore run in mode 2 (the same kernel, Householder always); K = 128 at 42 clones touches 40
of them and K = 64 / 65 at 43 clones touch 16.  The class is a property of d alone (tsqr_class), so the instantiation is the
one named, and n1 = 253 / 259 are reached by the other cases of the family.
"""
import functools

import numpy as np

import feature_cases as FC
import feature_reference as FR

LD = FR.LD
SIGMA2 = 0.035 ** 2               # default_ekf_cfg().noise_feature ** 2
# csrc/hip/ekf_limits.h; tests/test_update_limits.py holds these, the class functions and `predicted` against the header itself
# (all but LNB, which mirrors chol_block.h, a header that needs the HIP runtime: not checked)
IMU_DIM = 21
SU_MAX_NA, SU_CH = 24, 128
CHOL_LDS_MAX_ROWS, CHOL_PAN_RS, LNB = 181, 192, 16
TQ_THREADS = 512
TS_RB, TRSM_LPF = 16, 14
GEMM_TILE = 32
QR_BIAS_LIMIT = 1e-6

# the bars of tests/test_gpu_update_routes.py, all taken from the project
HH_P_BAR = 1e-12                  # test_ekf_update_householder_tsqr: Householder and uncompressed routes, against the plain reference
HH_X_BAR = 1e-9
GRAM_BAR = 1e-9                   # BASELINE's kernel-level bar: Gram route against update_with_prior, D_P and D_x
GRAM_PLAIN_BAR = 1e-6             # QR_BIAS_LIMIT: Gram route's D_P against the plain reference


# ---------------------------------------------------------------------------------------------- shapes
def chol_class(window):
    return 0 if 6 * window + 1 <= CHOL_LDS_MAX_ROWS else 1


def tsqr_class(window):
    return 0 if 6 * window + 1 <= 2 * (TQ_THREADS // 4) else 1


def l_fits(nk):
    return nk + TS_RB <= 16 * TRSM_LPF


def wide_rows_per_lane(window, n1):
    """RL of the tsqr_wide<4, RL> instantiation ekf_compress_exit takes for a stream alone in its launch: the row block has
    what the factorisation kernel's LDS leaves beside R (k_ekf_chol_lds) or the panel's space (k_ekf_chol)."""
    nt_d = 6 * window + 1
    if chol_class(window) == 0:
        room = nt_d * (nt_d + 1) // 2 + CHOL_PAN_RS * LNB - n1 * (n1 + 1) // 2
    else:
        room = LNB * ((nt_d + 15) // 16 * 16)
    assert room >= 16 * n1
    return 12 if room >= 48 * n1 else 8 if room >= 32 * n1 else 4


def predicted(route, mode, st, na, bias_flag):
    """used_qr of a stream from its shapes alone (k_ekf_small_update; ekf_compress_entry / ekf_compress_exit)."""
    hh = mode in (2, 3)
    if route == "small":
        return 1 if hh or (mode == 0 and (st <= na or bias_flag)) else 0
    if mode in (0, 3) and st <= na:
        return 2
    return 1 if hh or (mode == 0 and bias_flag) else 0


# ---------------------------------------------------------------------------------------------- problems
def split_rows(rows, n_active):
    """n_obs per feature such that sum(4 n_obs - 3) == rows, the runs cover n_active clones and no feature has more
    observations than there are active clones; features of three and more observations where that is possible (the gate
    of a two-observation feature has one degree of freedom and a threshold of 0.004), the fewest features otherwise."""
    for n_min in (3, 2):
        for k in range(1, rows):
            if (rows + 3 * k) % 4:
                continue
            total = (rows + 3 * k) // 4
            if total < max(n_active, n_min * k) or total > k * n_active:
                continue
            base, extra = divmod(total, k)
            return [base + 1] * extra + [base] * (k - extra)
    raise ValueError("no split of %d rows over %d clones" % (rows, n_active))


def P(family, route, window, active, rows, modes, limit, gap=None, bias="low", depth_scale=1.0, p_scale=1e-3, inflate=None, noise=5e-4, seed=0):
    active = tuple(range(window)) if active is None else tuple(active)
    return dict(family=family, route=route, window=window, active=active, rows=rows, modes=modes, limit=limit, gap=gap, bias=bias,
                depth_scale=depth_scale, p_scale=p_scale, inflate=inflate, noise=noise, seed=seed)


# Bias forced: the flag compares a BOUND, lambda max(P_aa) / sigma^2, with QR_BIAS_LIMIT.  Raising it with depth_scale and
# p_scale alone needs max diag(G) max(P) / sigma^2 >= 1e9 / d, an information ratio at which the double-precision oracle itself
# is 1e-12 .. 1e-9 away from the reference (measured: 1.2e-12 at best with the quantity at 14), beyond the Householder bar.
# The forced problems therefore make the bound loose instead: far features (depth_scale = 30, position columns of H around
# 1e-2) and the prior standard deviation of ONE position state, x of the last active clone, multiplied by `inflate` (750 ..
# 1500, chosen per window so that the quantity is 15 .. 22).  The update stays benign (oracle 1e-14 on the rest of P).  That
# variance (2e4 before, 1e2 after the update: three digits cancel in its own entry) dominates max|P|, so these cases are
# also judged on P' without its row and column, relative to what is left (distances(exclude=)).
def FORCED(inflate=1.5e3):
    return dict(bias="forced", depth_scale=30.0, inflate=inflate)


SCATTER = (0, 2, 3, 7, 11, 12, 18, 19, 23, 26, 29)
# name: family, route, window, active clones (None: all), stacked rows, {mode: used_qr}, limit
PROBLEMS = {
    "small3_w4": P("small3", "small", 4, (0, 1, 2), 27, {1: 0, 2: 1}, "np = 190: one Gram pair group; TSQR tree with one busy wavefront"),
    "small3_w30": P("small3", "small", 30, (5, 17, 29), 45, {1: 0, 2: 1}, "np = 190, d = 201"),
    "small4_w4_k39": P("small4", "small", 4, None, 39, {1: 0, 2: 1, 3: 1}, "np = 325: second pair slot; K < 128: three wavefronts idle"),
    "small4_w30_k598": P("small4", "small", 30, (26, 27, 28, 29), 598, {1: 0, 2: 1, 3: 1}, "512 < K < 640: blocks 2, 1, 1, 1, the last partial"),
    "small4_w64_k143": P("small4", "small", 64, (0, 21, 42, 63), 143, {1: 0, 2: 1, 3: 1}, "d = 405: second pass of the c += 256 loops"),
    "small4_w64_k13": P("small4", "small", 64, (0, 21, 42, 63), 13, {3: 1}, "st <= na in mode 3: the TSQR inside the fused kernel"),
    "smallbias_w12": P("smallbias", "small", 12, (2, 5, 8, 11), 39, {0: 1}, "s_bias gives need_qr", **FORCED()),
    "gen5_w5": P("first_general", "general", 5, None, 45, {1: 0, 3: 1}, "SU_MAX_NA + 6: n1 = 31, one GEMM tile; K inside one TSQR block"),
    "gen5_w30": P("first_general", "general", 30, (1, 8, 15, 22, 29), 45, {1: 0, 3: 1}, "n1 = 31 in a 201-wide state"),
    "gen6_w30": P("first_general", "general", 30, (1, 8, 15, 16, 22, 29), 51, {1: 0, 3: 1}, "n1 = 37: two GEMM tiles"),
    "lone97_w16": P("lone_residual", "general", 16, None, 113, {1: 0, 3: 1}, "n1 = 97: residual alone in the last GEMM tile and Cholesky panel; S 96 x 96"),
    "scatter_w30": P("scatter", "general", 30, SCATTER, 81, {1: 0, 3: 1}, "act[] is not the identity"),
    "scatter_w30_few": P("scatter", "general", 30, SCATTER, 45, {0: 2, 3: 2}, "st <= na, uncompressed, scattered columns"),
    "gap_w12": P("gated_gap", "general", 12, None, 85, {1: 0, 3: 1}, "rowmask-zero rows inside K", gap=4),
    "fallback_w10": P("fallback", "general", 10, None, 73, {0: 1}, "tsqr_wide<4, 12> (n1 = 61)", **FORCED()),
    "fallback_w15": P("fallback", "general", 15, None, 101, {0: 1}, "tsqr_wide<4, 8> (n1 = 91)", **FORCED()),
    "fallback_w30": P("fallback", "general", 30, None, 193, {0: 1}, "tsqr_wide<4, 4> at the LDS limit (n1 = 181)", **FORCED(1100.0)),
    "chol_w30": P("chol_edge", "general", 30, None, 193, {1: 0, 3: 1}, "k_ekf_chol_lds at nt = 181"),
    "chol_w31": P("chol_edge", "general", 31, None, 197, {1: 0, 3: 1}, "k_ekf_chol at nt = 187"),
    "chol_w31_bias": P("chol_edge", "general", 31, None, 197, {0: 1}, "fallback TSQR with R in the W buffer", **FORCED(750.0)),
    "lone193_w32": P("lone_residual_global", "general", 32, None, 205, {1: 0}, "n1 = 193: global Cholesky, last panel of one row"),
    "trsm_w34": P("trsm_edge", "general", 34, None, 217, {3: 1, 1: 0}, "l_fits at n = 204"),
    "trsm_w35": P("trsm_edge", "general", 35, None, 221, {3: 1, 1: 0}, "direct staging at n = 210"),
    "trsm_w35_few": P("trsm_edge", "general", 35, None, 209, {3: 2}, "uncompressed, nk = st = 209: direct staging, last block of one row"),
    "tsqr_w42_k128": P("tsqr_edge", "general", 42, tuple(c for c in range(42) if c not in (13, 30)), 128, {2: 1}, "<32,2,2>: one full block"),
    "tsqr_w42_k129": P("tsqr_edge", "general", 42, None, 129, {2: 1}, "<32,2,2>: a block of one row"),
    "tsqr_w42_k257": P("tsqr_edge", "general", 42, None, 257, {3: 1}, "<32,2,2> at n1 = 253, three blocks"),
    "tsqr_w43_k64": P("tsqr_edge", "general", 43, tuple(range(0, 43, 3)) + (41,), 64, {2: 1}, "<16,4,2>: one full block"),
    "tsqr_w43_k65": P("tsqr_edge", "general", 43, tuple(range(0, 43, 3)) + (41,), 65, {2: 1}, "<16,4,2>: a block of one row"),
    "tsqr_w43_k129": P("tsqr_edge", "general", 43, None, 129, {2: 1}, "<16,4,2> at n1 = 259, three blocks"),
    "tsqr_w43_k273": P("tsqr_edge", "general", 43, None, 273, {3: 1}, "<16,4,2> at n1 = 259, st > na"),
    "big_w64": P("largest_gram", "general", 64, None, 401, {1: 0}, "k_ekf_chol at nt = 385"),
}
for _i, _k in enumerate(sorted(PROBLEMS)):
    PROBLEMS[_k]["seed"] = 500 + _i
# problems that got another seed (test_update_cases: the oracle alone must stay within one eighth of the bar): none so far
RESEEDED = {}
for _k, _s in RESEEDED.items():
    PROBLEMS[_k]["seed"] = _s

CASES = {"%s_m%d" % (k, m): (k, m) for k in sorted(PROBLEMS) for m in sorted(PROBLEMS[k]["modes"])}
FAMILIES = sorted(set(p["family"] for p in PROBLEMS.values()))


@functools.lru_cache(maxsize=None)
def problem(pname):
    """The feature_cases case dict of a problem, with active, na, n1, st, K, rows_of, gated (feature indices placed as outliers)."""
    from oracle import oracle_py as O
    p = PROBLEMS[pname]
    act = sorted(p["active"])
    n_obs = split_rows(p["rows"], len(act))
    specs, off = [], 0
    for n in n_obs:
        specs.append(FC.spec(sorted(act[(off + i) % len(act)] for i in range(n)), needs_init=0))
        off += n
    gated = []
    if p["gap"]:
        mid = len(specs) // 2
        specs.insert(mid, FC.spec(act[:p["gap"]], needs_init=0, outlier=True))
        gated = [mid]
    c = FC.build_case(O.euroc_calib(376, 240), pname, p["seed"], p["window"], specs, noise=p["noise"], depth_scale=p["depth_scale"])
    c = dict(c)
    c["P"] = c["P"] * (p["p_scale"] / 1e-3)
    c["inflated"] = None
    if p["inflate"]:
        c["inflated"] = IMU_DIM + 6 * act[-1] + 3
        D = np.ones(len(c["P"]))
        D[c["inflated"]] = p["inflate"]
        c["P"] = c["P"] * D[:, None] * D[None, :]
    rows_of = np.array([4 * len(s["jac"]) - 3 for s in specs])
    stacked = np.ones(len(specs), bool)
    stacked[gated] = False
    ends = np.cumsum(rows_of)
    c.update(active=act, na=6 * len(act), n1=6 * len(act) + 1, st=int(rows_of[stacked].sum()), K=int(ends[np.flatnonzero(stacked)[-1]]),
             rows_of=rows_of, gated=gated, stacked=stacked, d=IMU_DIM + 6 * p["window"], **{k: p[k] for k in ("family", "route", "limit", "bias", "modes")})
    assert c["st"] == p["rows"]
    return c


def case(name):
    """A case: its problem's dict + name, mode, used_qr, gram."""
    pname, mode = CASES[name]
    c = dict(problem(pname))
    c.update(name=name, problem=pname, mode=mode, used_qr=c["modes"][mode], gram=c["modes"][mode] == 0)
    return c


def act_columns(c):
    return np.concatenate([IMU_DIM + 6 * ci + np.arange(6) for ci in c["active"]])


# ---------------------------------------------------------------------------------------------- the reference
@functools.lru_cache(maxsize=None)
def stack(pname):
    """Long-double gate of every feature and the stacked (H, r) of the passing ones, in feature order."""
    c = problem(pname)
    chi2 = FR.chi2_table()
    n = len(c["specs"])
    gamma, passed, blocks = np.zeros(n, dtype=LD), np.zeros(n, bool), []
    for j in range(n):
        oc, oz = FC.obs_of(c, j)
        g = FR.feature_gate(c["calib"], c["clones"], c["P"], c["positions"][j], oc, oz, c["gravity"], SIGMA2)
        gamma[j] = np.inf if g["gamma"] is None else g["gamma"]
        passed[j] = FR.passes(g["gamma"], len(oc), c["dof_offset"], chi2)
        if passed[j]:
            blocks.append((g["H_o"], g["r_o"]))
    H = np.vstack([b[0] for b in blocks])
    r = np.concatenate([b[1] for b in blocks])
    dof = np.array([len(s["jac"]) + c["dof_offset"] for s in c["specs"]])
    return dict(gamma=gamma, passed=passed, H=H, r=r, margin=gamma / chi2[dof])


def lam_of(c, H):
    """lambda = 1e-14 d max diag(H_act^T H_act), from the reference's H."""
    Ha = np.asarray(H, dtype=LD)[:, act_columns(c)]
    return LD(1e-14) * c["d"] * (Ha * Ha).sum(0).max()


def bias_quantity(pname):
    """1e-14 d max diag(G) max P_aa / (1e-6 sigma^2): what the factorisation kernels compare with 1 for the bias flag."""
    c = problem(pname)
    cols = act_columns(c)
    return float(lam_of(c, stack(pname)["H"]) * np.diag(c["P"])[cols].max() / (QR_BIAS_LIMIT * SIGMA2))


def update_plain(c, H, r):
    return FR.update(c["P"], [(H, r)], SIGMA2)


def update_with_prior(c, H, r):
    """The same update with na extra rows sqrt(lambda) e_act(i) and zero residual."""
    cols = act_columns(c)
    E = np.zeros((len(cols), c["d"]), dtype=LD)
    E[np.arange(len(cols)), cols] = np.sqrt(lam_of(c, H))
    return FR.update(c["P"], [(H, r), (E, np.zeros(len(cols), dtype=LD))], SIGMA2)


@functools.lru_cache(maxsize=None)
def reference(pname):
    """(delta_x, P') of the plain long-double update."""
    s = stack(pname)
    return update_plain(problem(pname), s["H"], s["r"])


@functools.lru_cache(maxsize=None)
def reference_with_prior(pname):
    s = stack(pname)
    return update_with_prior(problem(pname), s["H"], s["r"])


def distances(dx, Pn, ref, exclude=None):
    """(D_P, D_x) = max|dP| / max|P_ref|, max|d delta_x| / max|delta_x_ref|; exclude: a state whose row and column of P (and
    entry of delta_x) are left out of both the difference and the scale."""
    dx_ref, P_ref = ref
    if exclude is not None:
        keep = np.arange(len(dx_ref)) != exclude
        dx, Pn, dx_ref, P_ref = np.asarray(dx)[keep], np.asarray(Pn)[np.ix_(keep, keep)], dx_ref[keep], P_ref[np.ix_(keep, keep)]
    D_P = float(np.abs(np.asarray(Pn, dtype=LD) - P_ref).max() / np.abs(P_ref).max())
    D_x = float(np.abs(np.asarray(dx, dtype=LD) - dx_ref).max() / np.abs(dx_ref).max())
    return D_P, D_x


def gram_double(c, H, r):
    """The Gram algebra of the kernels in plain numpy double (G + lambda I, Cholesky, T, S, solve, downdate): not the code
    under test, only the proof that the Gram bar can be met in double arithmetic."""
    from scipy.linalg import solve_triangular
    cols = act_columns(c)
    Ha, rr, Pd = np.asarray(H, dtype=np.float64)[:, cols], np.asarray(r, dtype=np.float64), np.asarray(c["P"], dtype=np.float64)
    G = Ha.T @ Ha
    lam = 1e-14 * c["d"] * np.diag(G).max()
    L = np.linalg.cholesky(G + lam * np.eye(len(cols)))
    w = solve_triangular(L, Ha.T @ rr, lower=True)                 # Q^T r
    T = L.T @ Pd[cols, :]
    S = T[:, cols] @ L + SIGMA2 * np.eye(len(cols))
    L2 = np.linalg.cholesky((S + S.T) / 2)
    Y = solve_triangular(L2, np.hstack([T, w[:, None]]), lower=True)
    Pn = Pd - Y[:, :-1].T @ Y[:, :-1]
    return Y[:, :-1].T @ Y[:, -1], (Pn + Pn.T) / 2


def oracle_update(oracle, c):
    """The double-precision oracle's update of the whole problem (Householder compression)."""
    from msckf_stereo_c_amd.ctypes_types import default_ekf_cfg
    return oracle.ekf_update_problem(c["calib"], default_ekf_cfg(max_cam_state_size=c["window"]), c["gravity"], c["clones"], c["P"], c["positions"],
                                     c["obs_start"], c["obs_clone"], c["obs_z"], c["dof_offset"])
