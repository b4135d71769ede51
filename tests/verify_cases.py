"""Jobs of the geometric verification ("Geometric verification") for tests/test_verify_reference.py and
tests/test_gpu_verify.py: seeded scenes with a planted pose (an EuRoC-like T_cam1_cam0, points 1 .. 15 m ahead of the query's
cam0) at the sizes where k_fe_verify takes another path, and hand-made jobs with the answer written beside each (`want`)."""
import numpy as np

import verify_reference as VR

FX = 458.0                                # pixels per normalised unit of the scenes: "0.5 px" is 0.5 / FX
MAX_ERROR = 2.0 / FX
MIN_DEPTH, MAX_DEPTH = 0.1, 40.0


def rot(axis, angle):
    """Rodrigues (test data only: the contract itself uses no transcendental)."""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def T_of(R, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T


T10 = T_of(rot([0.3, 1.0, -0.2], 0.004), [-0.110074, 0.000399, -0.000853])       # EuRoC-like: 11 cm to the right, nearly parallel


def observe(T, p):
    """(x0, y0, x1, y1) of points p[n, 3] in a cam0 frame."""
    q = p @ T[:3, :3].T + T[:3, 3]
    return np.stack([p[:, 0] / p[:, 2], p[:, 1] / p[:, 2], q[:, 0] / q[:, 2], q[:, 1] / q[:, 2]], axis=1)


def points(rng, n, z0=1.0, z1=15.0):
    z = rng.uniform(z0, z1, n)
    return np.stack([rng.uniform(-0.45, 0.45, n) * z, rng.uniform(-0.3, 0.3, n) * z, z], axis=1)


def scene(seed, n, wrong=0.0, noise_px=0.0, R=None, t=None):
    """n pairs under the planted motion p_k = R p_q + t: (query_obs, train_obs, is_wrong bool[n], R, t).  A wrong pair's keyframe
    observation is that of another random point; noise is Gaussian on all eight coordinates."""
    rng = np.random.default_rng([seed, n])
    R = rot([0.2, 1.0, 0.1], 0.06) if R is None else R
    t = np.array([0.25, -0.05, 0.4]) if t is None else np.asarray(t, np.float64)
    p = points(rng, n)
    pk = p @ R.T + t
    is_wrong = rng.uniform(size=n) < wrong
    if n:
        pk[is_wrong] = points(rng, int(is_wrong.sum()))
    q, k = observe(T10, p), observe(T10, pk)
    if noise_px:
        q = q + rng.normal(0, noise_px / FX, q.shape)
        k = k + rng.normal(0, noise_px / FX, k.shape)
    return np.ascontiguousarray(q), np.ascontiguousarray(k), is_wrong, R, t


def case(name, q, k, usable=None, K=64, seed=1, max_error=MAX_ERROR, want=None, **extra):
    c = dict(name=name, query_obs=np.ascontiguousarray(q, np.float64).reshape(-1, 4), train_obs=np.ascontiguousarray(k, np.float64).reshape(-1, 4),
             usable=None if usable is None else np.ascontiguousarray(usable, np.uint8), T_cam1_cam0=T10.copy(), n_hypotheses=K, seed=seed, max_error=max_error,
             min_depth=MIN_DEPTH, max_depth=MAX_DEPTH, want=want)
    c.update(extra)
    for a in (c["query_obs"], c["train_obs"], c["T_cam1_cam0"]):
        a.setflags(write=False)
    return c


def options(c):
    """The keyword arguments of VR.verify / Context.verify of a case."""
    return {k: c[k] for k in ("query_obs", "train_obs", "T_cam1_cam0", "max_error", "usable", "n_hypotheses", "seed", "min_depth", "max_depth")}


# ------------------------------------------------------------------------------------------ sizes (all pairs usable)
# usable n at the wavefront (64) and tile (VR.TILE) edges, K at the workgroup (64) edges
SIZES = [(3, 1), (4, 63), (63, 64), (64, 65), (65, 256), (VR.TILE - 1, 1024), (VR.TILE, 64), (VR.TILE + 1, 65), (437, 256), (4096, 1024), (2 * VR.TILE + 1, 63), (4096, 1)]
CASES = []
for _n, _K in SIZES:
    _q, _k, _w, _, _ = scene(100 + _K, _n, wrong=0.3 if _n >= 63 else 0.0, noise_px=0.3)
    CASES.append(case("size %dx%d" % (_n, _K), _q, _k, K=_K, seed=_n + _K, is_wrong=_w))

# ------------------------------------------------------------------------------------------ hand-made
NO_HYPOTHESIS = dict(best=-1, n_inliers=0, status=1)
for _n in (0, 1, 2):
    _q, _k, _, _, _ = scene(7, _n)
    CASES.append(case("n = %d" % _n, _q, _k, want=dict(NO_HYPOTHESIS, n_usable=_n)))

_q, _k, _, _, _ = scene(8, 1)
CASES.append(case("three identical points", np.repeat(_q, 3, axis=0), np.repeat(_k, 3, axis=0), want=dict(NO_HYPOTHESIS, n_usable=3)))

# every point on one line through (0.3, -0.2, 2) in the query frame: every sample triangle is flat
_s = np.linspace(0.0, 6.0, 20)[:, None]
_p = np.array([0.3, -0.2, 2.0]) + _s * np.array([0.1, 0.05, 1.0])
_R, _t = rot([0.2, 1.0, 0.1], 0.06), np.array([0.25, -0.05, 0.4])
CASES.append(case("all points collinear", observe(T10, _p), observe(T10, _p @ _R.T + _t), want=dict(NO_HYPOTHESIS, n_usable=20)))

# noise-free, no wrong pair: every non-void hypothesis counts all 40 pairs, so the lowest non-void h wins (the tie rule); a thin
# but non-void sample triangle amplifies the observations' rounding (1e-16) by far less than the threshold's 4e-3
_q, _k, _, _, _ = scene(9, 40)
CASES.append(case("noise-free, no outliers", _q, _k, K=64, seed=3, want=dict(n_usable=40, n_inliers=40, status=0), lowest_non_void=True))

# the keyframe camera stands 5 m ahead of the query's: the points nearer than that lie behind it.  Their keyframe observations
# (a real camera has none) are those of other points, so the pairs are usable; the threshold is enormous, so under the planted
# motion every pair in front is an inlier and none behind is
_rng = np.random.default_rng(10)
_p = points(_rng, 60)
_tb = np.array([0.0, 0.0, -5.0])
_pk = _p + _tb
_pk1 = _pk @ T10[:3, :3].T + T10[:3, 3]
BEHIND = (_pk[:, 2] < MIN_DEPTH) | (_pk1[:, 2] < MIN_DEPTH)
_pk_seen = np.where(BEHIND[:, None], points(_rng, 60), _pk)
assert 10 <= BEHIND.sum() <= 50 and min(np.abs(_pk[:, 2] - MIN_DEPTH).min(), np.abs(_pk1[:, 2] - MIN_DEPTH).min()) > 1e-3       # (no point on the edge)
CASES.append(case("points behind the keyframe camera", observe(T10, _p), observe(T10, _pk_seen), K=256, seed=4, max_error=1e3, behind=BEHIND,
                  want=dict(n_usable=60, status=0)))

# a usable mask, zero-disparity observations (x1, y1 = the projection of the ray's direction: A.A = 0 or the depth beyond any
# bound) and points 100 m away (beyond max_depth), on either side of the pair: never sampled, never inliers
_q, _k, _, _, _ = scene(11, 50)
_q, _k = _q.copy(), _k.copy()
MASKED = np.zeros(50, bool)
MASKED[[0, 7, 49]] = True
_dirs = np.concatenate([np.stack([_q[3, :2], _k[4, :2]]), np.ones((2, 1))], axis=1)
_far = _dirs @ T10[:3, :3].T
_q[3, 2:], _k[4, 2:] = _far[0, :2] / _far[0, 2], _far[1, :2] / _far[1, 2]
_q[5], _k[6] = observe(T10, np.array([[3.0, 1.0, 100.0]]))[0], observe(T10, np.array([[-2.0, 1.0, 90.0]]))[0]
UNUSABLE = MASKED.copy()
UNUSABLE[[3, 4, 5, 6]] = True
CASES.append(case("usable mask and zero disparity", _q, _k, usable=(~MASKED).astype(np.uint8), K=64, seed=5, unusable=UNUSABLE,
                  want=dict(n_usable=43, n_inliers=43, status=0)))

# the property test's input: 437 pairs, half of them wrong, 0.5 px noise, 256 hypotheses
_q, _k, _w, PLANTED_R, PLANTED_T = scene(12, 437, wrong=0.5, noise_px=0.5)
CASES.append(case("planted 437, half wrong", _q, _k, K=256, seed=2026, is_wrong=_w))

# a small noisy job for the threshold sweep and the slow loop
_q, _k, _w, _, _ = scene(13, 48, wrong=0.25, noise_px=0.5)
CASES.append(case("noisy 48", _q, _k, K=32, seed=6, is_wrong=_w))

BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)
