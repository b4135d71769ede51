"""Seeded update problems that drive the measurement update's per-feature stage (triangulate_wave, k_ekf_triangulate, the
three instantiations of k_ekf_feature_blocks, k_ekf_pair_blocks) at its triangulation, validity and size-class edges.

Every case starts from ekf_problems.make_problem with min_obs = n_clones, so that every feature is observed by every clone
of the window; a feature of the case then picks the clones of its Jacobian block (n_obs) and, when it is to be triangulated
on the device, the clones of its triangulation (n_init) from those observations.  Three seeded alterations of a feature's
observations put it where the case needs it:

  outlier : the middle Jacobian observation is moved by 1.0 in y (both cameras): the feature is gated out (and its triangulation
            meets the Huber weight);
  behind  : its observations are the (noise-free) projections of the point mirrored at the first clone, which lies
            behind every camera: the triangulation converges there and is invalid;
  far sets (depth_scale = 30, features at 90 - 240 m) carry invalid triangulations of their own.

A case is a dict:
  name, variant ("pair" | "wave" | "mixed": what the stream's route is), window, calib, dof_offset, apply_row_cap,
  clones, P, gravity, positions (the given positions: used where needs_init is 0),
  obs_start / obs_clone / obs_z   : the Jacobian observations, contiguous (what the oracle and the reference read),
  needs_init, init_start / init_clone / init_z : the triangulation observations, contiguous (an empty range where
                                    needs_init is 0),
  cls                             : per feature the kernel variant that handles it ("pair", "wave", "small", "big"),
  dev                             : the device layout, as buildPruneUpdate lays a feature out: its triangulation
                                    observations first, its Jacobian observations behind them; dict(obs_clone, obs_z,
                                    obs_start, n_obs, init_ranges).

tests/test_feature_cases.py holds the conditions that keep these sets from degenerating and measures the bars (no GPU);
tests/test_gpu_feature_edges.py runs them on the device.
"""
import copy
import functools
import math

import numpy as np

import ekf_problems
import feature_reference as FR

FEAT_WAVE_CLONES, FEAT_SMALL_CLONES, TRI_SMALL_CLONES = 4, 16, 32       # csrc/hip/ekf_limits.h
GATE_LDS_ROWS = 120                                                    # ekf_kernels.hip: 30 observations fit, 31 do not
EKF_SLOTS = 64
FAR = dict(depth_scale=30.0)


def wide_stereo_calib(calib, yaw_deg=75.0):
    """The calibration with cam1 turned by yaw_deg about y: features on one side of cam0 lie BEHIND cam1."""
    c = copy.deepcopy(calib)
    T = np.array(calib.T_cam1_cam0).reshape(4, 4).copy()
    a = math.radians(yaw_deg)
    T[:3, :3] = np.array([[math.cos(a), 0, math.sin(a)], [0, 1.0, 0], [-math.sin(a), 0, math.cos(a)]])
    c.T_cam1_cam0[:] = list(T.reshape(-1))
    return c


def spec(jac, init=None, needs_init=1, outlier=False, behind=False):
    return dict(jac=tuple(jac), init=tuple(jac if init is None else init), needs_init=needs_init, outlier=outlier, behind=behind)


def pick(rng, window, n_obs, n_init=None):
    """(Jacobian clones, triangulation clones): n_obs random clones, ascending; the triangulation takes those and further
    random clones up to n_init (the first n_init of them when n_init < n_obs)."""
    jac = sorted(int(c) for c in rng.choice(window, n_obs, replace=False))
    if n_init is None or n_init == n_obs:
        return jac, jac
    if n_init < n_obs:
        return jac, jac[:n_init]
    others = [c for c in range(window) if c not in jac]
    more = [int(c) for c in rng.choice(others, n_init - n_obs, replace=False)]
    return jac, sorted(jac + more)


def stream_variant(specs):
    """What plan_stream (mskf_capi_ekf.cpp) decides for a stream of these features."""
    pairs = all(len(s["jac"]) == 2 and s["jac"] == specs[0]["jac"] and s["jac"][0] < s["jac"][1] for s in specs)
    if pairs:
        return "pair"
    if all(len(s["jac"]) <= FEAT_WAVE_CLONES and (not s["needs_init"] or len(s["init"]) <= TRI_SMALL_CLONES) for s in specs):
        return "wave"
    return "mixed"


def build_case(calib, name, seed, window, specs, noise=0.002, depth_scale=1.0, dof_offset=-1):
    n_feat = len(specs)
    pr = ekf_problems.make_problem(calib, seed=seed, n_clones=window, n_feat=n_feat, min_obs=window, noise=noise, depth_scale=depth_scale)
    assert len(pr["obs_clone"]) == n_feat * window
    z = pr["obs_z"].reshape(n_feat, window, 4).copy()
    T01 = np.array(calib.T_cam1_cam0).reshape(4, 4)
    for j, s in enumerate(specs):
        if s["outlier"]:
            z[j, s["jac"][len(s["jac"]) // 2], 1] += 1.0         # (not the last view where there are three: the initial guess starts there)
            z[j, s["jac"][len(s["jac"]) // 2], 3] += 1.0
        if s["behind"]:
            mirrored = 2 * pr["clones"][0, 4:7] - pr["positions"][j]
            for c in range(window):
                pc0 = ekf_problems.quat_to_rot(pr["clones"][c, 0:4]) @ (mirrored - pr["clones"][c, 4:7])
                pc1 = T01[:3, :3] @ pc0 + T01[:3, 3]
                z[j, c] = [pc0[0] / pc0[2], pc0[1] / pc0[2], pc1[0] / pc1[2], pc1[1] / pc1[2]]
    variant = stream_variant(specs)
    obs_start, obs_clone, obs_z = [0], [], []
    init_start, init_clone, init_z = [0], [], []
    dev = dict(obs_clone=[], obs_z=[], obs_start=[], n_obs=[], init_ranges=[])
    cls = []
    for j, s in enumerate(specs):
        if s["needs_init"]:
            dev["init_ranges"].append((len(dev["obs_clone"]), len(s["init"])))
            for c in s["init"]:
                init_clone.append(c); init_z.append(z[j, c])
                dev["obs_clone"].append(c); dev["obs_z"].append(z[j, c])
        else:
            dev["init_ranges"].append((0, 0))
        init_start.append(len(init_clone))
        dev["obs_start"].append(len(dev["obs_clone"]))
        dev["n_obs"].append(len(s["jac"]))
        for c in s["jac"]:
            obs_clone.append(c); obs_z.append(z[j, c])
            dev["obs_clone"].append(c); dev["obs_z"].append(z[j, c])
        obs_start.append(len(obs_clone))
        size = max(len(s["jac"]), len(s["init"]) if s["needs_init"] else 0)
        cls.append(variant if variant != "mixed" else ("small" if size <= FEAT_SMALL_CLONES else "big"))
    dev = dict(obs_clone=np.array(dev["obs_clone"], np.int32), obs_z=np.array(dev["obs_z"]).reshape(-1, 4),
               obs_start=np.array(dev["obs_start"], np.int32), n_obs=np.array(dev["n_obs"], np.int32), init_ranges=dev["init_ranges"])
    return dict(name=name, variant=variant, window=window, calib=calib, dof_offset=dof_offset, apply_row_cap=dof_offset < 0, specs=specs,
                clones=pr["clones"], P=pr["P"], gravity=pr["gravity"], positions=pr["positions"],
                obs_start=np.array(obs_start, np.int32), obs_clone=np.array(obs_clone, np.int32), obs_z=np.array(obs_z).reshape(-1, 4),
                needs_init=np.array([s["needs_init"] for s in specs], np.int32),
                init_start=np.array(init_start, np.int32), init_clone=np.array(init_clone, np.int32), init_z=np.array(init_z).reshape(-1, 4),
                cls=cls, dev=dev)


# ---------------------------------------------------------------------------------------------- the cases
def _pair(calib, name, seed, window, pair, n_feat, n_inits, skip_every, behind):
    """Pruning shape: every Jacobian block is the ascending pair; the triangulation covers n_init clones around it."""
    specs = []
    for j in range(n_feat):
        k = n_inits[j % len(n_inits)]
        start = max(0, min(pair[0], window - k))
        specs.append(spec(pair, range(start, start + k), needs_init=0 if j % skip_every == skip_every - 1 else 1, behind=j in behind))
    return build_case(calib, name, seed, window, specs, noise=0.004, dof_offset=0, **FAR)


def _wave(calib, name, seed, window, n_feat, n_inits, behind=(), leave=None, noise=0.003, depth_scale=30.0, all_init=False):
    rng = np.random.default_rng(seed + 1000)
    specs = []
    for j in range(n_feat):
        n_obs = (2, 3, 4)[j % 3]
        k = n_inits[j % len(n_inits)]
        jac, init = pick(rng, window, n_obs, k)
        if leave is not None and j == leave[0]:
            jac, init = pick(np.random.default_rng(seed + 2000), window, n_obs, leave[1])
        specs.append(spec(jac, init, needs_init=0 if (j % 8 == 7 and not all_init) else 1, outlier=j % 9 == 3, behind=j in behind))
    return build_case(calib, name, seed, window, specs, noise=noise, depth_scale=depth_scale, dof_offset=0)


def _classes(calib, name, seed, window, rows):
    """rows = [(n_obs, n_init or None, kinds)]: one feature per kind, "p" plain, "o" outlier, "b" behind, "g" position given."""
    rng = np.random.default_rng(seed + 1000)
    specs = []
    for n_obs, n_init, kinds in rows:
        for kind in kinds:
            jac, init = pick(rng, window, n_obs, n_init)
            specs.append(spec(jac, init, needs_init=0 if kind == "g" else 1, outlier=kind == "o", behind=kind == "b"))
    return build_case(calib, name, seed, window, specs, noise=0.002, **FAR)


def _slots(calib, name, seed, window, n_obs, n_feat):
    """n_feat members of one class in one stream: group s of the launch handles features s, s + 64, s + 128.  Groups 0..3
    see [invalid, pass], [pass, invalid], [gated-out, pass], [pass, gated-out] in turn."""
    rng = np.random.default_rng(seed + 1000)
    specs = []
    for j in range(n_feat):
        slot, rnd = j % EKF_SLOTS, j // EKF_SLOTS
        jac, init = pick(rng, window, n_obs)
        specs.append(spec(jac, init, behind=(slot, rnd) in ((0, 0), (1, 1)), outlier=(slot, rnd) in ((2, 0), (3, 1))))
    return build_case(calib, name, seed, window, specs, noise=0.002, **FAR)


CASES = {
    # k_ekf_triangulate + k_ekf_pair_blocks
    "pair_w12_65": lambda c: _pair(c, "pair_w12_65", 6, 12, (3, 4), 65, (1, 2, 3, 12), 6, (0, 64)),
    "pair_w64_129": lambda c: _pair(c, "pair_w64_129", 7, 64, (30, 31), 129, (1, 2, 3, 32, 33, 64), 7, (0, 64, 128)),
    # k_ekf_feature_blocks<4, true, 256>: 5, 65 and 257 features leave one wavefront of the last workgroup busy
    "wave_w12_5": lambda c: _wave(c, "wave_w12_5", 11, 12, 5, (None,), noise=0.002, depth_scale=1.0, all_init=True),
    "wave_w30_65": lambda c: _wave(c, "wave_w30_65", 12, 30, 65, (None, 5, 16, 17), behind=(1,)),
    "wave_w64_257": lambda c: _wave(c, "wave_w64_257", 13, 64, 257, (None, 5, 16, 17, 32), behind=(2, 256)),
    "wave_w64_257_leaves": lambda c: _wave(c, "wave_w64_257_leaves", 13, 64, 257, (None, 5, 16, 17, 32), behind=(2, 256), leave=(100, 33)),
    "wide_stereo_w12": lambda c: _wave(wide_stereo_calib(c), "wide_stereo_w12", 14, 12, 24, (None,), noise=0.001, depth_scale=1.0, all_init=True),
    # k_ekf_feature_blocks<16, false, 64>
    "small_w30": lambda c: _classes(c, "small_w30", 21, 30, [(5, None, "pobg"), (16, None, "pobg"), (5, 16, "pob")]),
    # k_ekf_feature_blocks<32, false, 256> / <64, false, 256>
    "big_w30": lambda c: _classes(c, "big_w30", 22, 30, [(17, None, "pob"), (29, None, "po"), (30, None, "po")]),
    "big_w32": lambda c: _classes(c, "big_w32", 23, 32, [(17, None, "pob"), (30, None, "pob"), (31, None, "pob"), (32, None, "pobg"), (5, 17, "pb")]),
    "big_w64": lambda c: _classes(c, "big_w64", 24, 64, [(33, None, "pob"), (63, None, "po"), (64, None, "pog"), (5, 17, "p"),
                                                         (30, None, "pob"), (31, None, "pob")]),
    # more than EKF_SLOTS members of one class in one stream
    "slots_small_65": lambda c: _slots(c, "slots_small_65", 31, 12, 5, 65),
    "slots_small_129": lambda c: _slots(c, "slots_small_129", 32, 12, 5, 129),
    "slots_big_65": lambda c: _slots(c, "slots_big_65", 33, 32, 31, 65),
    "slots_big_129": lambda c: _slots(c, "slots_big_129", 34, 32, 31, 129),
}
FAR_SETS = ("pair_w12_65", "pair_w64_129", "wave_w30_65", "wave_w64_257")


@functools.lru_cache(maxsize=None)
def case(name):
    from oracle import oracle_py as O
    return CASES[name](O.euroc_calib(376, 240))


def obs_of(c, j):
    sl = slice(c["obs_start"][j], c["obs_start"][j + 1])
    return c["obs_clone"][sl], c["obs_z"][sl]


def init_of(c, j):
    sl = slice(c["init_start"][j], c["init_start"][j + 1])
    return c["init_clone"][sl], c["init_z"][sl]


def init_problem(c):
    """(indices of the needs_init features, obs_start over them alone): the triangulation observations as one contiguous
    problem (the empty ranges of the other features drop out)."""
    idx = np.flatnonzero(c["needs_init"])
    return idx, np.concatenate([[0], c["init_start"][idx + 1]]).astype(np.int32)


def sub_problem(c, keep):
    """The Jacobian observations of the features `keep` (indices, ascending) as a contiguous problem of their own."""
    obs_start, oc, oz = [0], [], []
    for j in keep:
        a, b = obs_of(c, j)
        oc.append(a); oz.append(b)
        obs_start.append(obs_start[-1] + len(a))
    if not oc:
        return np.array(obs_start, np.int32), np.zeros(0, np.int32), np.zeros((0, 4))
    return np.array(obs_start, np.int32), np.concatenate(oc), np.concatenate(oz)


def oracle_update(oracle, c, positions, keep):
    """The CPU oracle's update of the features `keep` at `positions` (n_feat x 3): its result dict, gamma / passed scattered
    back to the case's feature indices (gamma -1, passed 0 where the oracle did not evaluate or was not asked)."""
    from msckf_stereo_c_amd.ctypes_types import default_ekf_cfg
    keep = [int(j) for j in keep]
    obs_start, oc, oz = sub_problem(c, keep)
    cfg = default_ekf_cfg(max_cam_state_size=c["window"])
    r = oracle.ekf_update_problem(c["calib"], cfg, c["gravity"], c["clones"], c["P"], np.asarray(positions, dtype=np.float64)[keep],
                                  obs_start, oc, oz, c["dof_offset"])
    n = len(c["cls"])
    gamma, passed = np.full(n, -1.0), np.zeros(n, np.uint8)
    gamma[keep], passed[keep] = r["gamma"], r["passed"]
    return dict(rows=r["rows"], gamma=gamma, passed=passed, delta_x=r["delta_x"], P=r["P"])


@functools.lru_cache(maxsize=None)
def reference_triangulation(name):
    """Long-double triangulation of every needs_init feature of the case: list of feature_reference.triangulate results
    (None where the position is given)."""
    c = case(name)
    return [FR.triangulate(c["calib"], c["clones"], *init_of(c, j)) if c["needs_init"][j] else None for j in range(len(c["cls"]))]


def reference_gates(c, positions, sigma2, chi2, only=None, mutate=None):
    """Long-double gamma and pass bit of the features `only` (default: all) at the given positions -> (gamma, passed), NaN /
    False where a feature was not asked for."""
    n = len(c["cls"])
    gamma, passed = np.full(n, np.nan, dtype=FR.LD), np.zeros(n, bool)
    for j in (range(n) if only is None else only):
        oc, oz = obs_of(c, j)
        g = FR.feature_gate(c["calib"], c["clones"], c["P"], positions[j], oc, oz, c["gravity"], sigma2, mutate)
        gamma[j] = np.inf if g["gamma"] is None else g["gamma"]
        passed[j] = FR.passes(g["gamma"], len(oc), c["dof_offset"], chi2, mutate)
    return gamma, passed
