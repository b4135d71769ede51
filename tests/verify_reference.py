"""The geometric verification's contract ("Geometric verification"; csrc/hip/fe_verify.h) restated in Python,
operation for operation in IEEE double: Python floats where one hypothesis or one pair is at work, numpy float64 arrays (element-wise
operations only: no dot, no matmul, nothing a library could contract or reorder) where one hypothesis meets every pair.  Sums go
left to right exactly as the header writes them; only + - * / and sqrt are used, so the results are equal bit for bit.

`verify(...)` is the whole job as mskf_fe_verify returns it.  MISTAKES names deliberate deviations for the tests that must catch
them: verify(..., mistake=name)."""
import math

import numpy as np

MAX_N, MAX_K, TILE, PAIR, HYP_BLOCK = 4096, 1024, 256, 7, 64
MIN_SIN2 = 1e-4
REFINE_ITERS = 5
KEY_NONE = 0
DRAW_C = 0x5FE7E21F5FE7E21F
M64 = (1 << 64) - 1
MISTAKES = ("non-strict threshold", "highest-h tie", "R transposed", "cam1 residuals dropped", "draws not distinct", "void triads scored")


def cam_of(T):
    """(R10 as 9 floats row-major, t10 as 3 floats) of a row-major 4x4."""
    T = [float(v) for v in np.asarray(T, dtype=np.float64).reshape(-1)]
    return [T[4 * i + j] for i in range(3) for j in range(3)], [T[4 * i + 3] for i in range(3)]


def dot3(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def mat_vec(M, v):
    return [(M[3 * i] * v[0] + M[3 * i + 1] * v[1]) + M[3 * i + 2] * v[2] for i in range(3)]


def cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _div(a, b):
    """IEEE division of Python floats (b = 0 gives inf / nan as in C, where Python raises)."""
    return float(np.float64(a) / np.float64(b))


# ------------------------------------------------------------------------------------------ triangulation and staging
def triangulate(cam, o):
    """depth of the cam0 ray, or None where A.A is not > 0."""
    R, t = cam
    m = mat_vec(R, [o[0], o[1], 1.0])
    a0, a1 = m[0] - o[2] * m[2], m[1] - o[3] * m[2]
    b0, b1 = o[2] * t[2] - t[0], o[3] * t[2] - t[1]
    aa, ab = a0 * a0 + a1 * a1, a0 * b0 + a1 * b1
    if not aa > 0.0:
        return None
    return _div(ab, aa)


def usable_point(cam, o, min_depth, max_depth):
    with np.errstate(all="ignore"):
        d = triangulate(cam, o)
    if d is None or not (d >= min_depth and d <= max_depth):
        return None
    return [o[0] * d, o[1] * d, d]


def stage(cam, query_obs, train_obs, usable, min_depth, max_depth):
    """(pairs float64[m, 7], orig int[m]): the usable pairs in order and their original indices."""
    pairs, orig = [], []
    for i in range(len(query_obs)):
        if usable is not None and not usable[i]:
            continue
        q = [float(v) for v in query_obs[i]]
        k = [float(v) for v in train_obs[i]]
        a, pk = usable_point(cam, q, min_depth, max_depth), usable_point(cam, k, min_depth, max_depth)
        if a is None or pk is None:
            continue
        pairs.append(a + k)
        orig.append(i)
    return np.array(pairs, np.float64).reshape(-1, PAIR), np.array(orig, np.int64)


# ------------------------------------------------------------------------------------------ draws
def mix(z):
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & M64
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    return z


def rand(seed, k):
    return mix((mix((seed + DRAW_C) & M64) + 0x9E3779B97F4A7C15 * k) & M64)


def draw(seed, h, n, mistake=None):
    """Three distinct indices 0 .. n - 1 of hypothesis h (n >= 3)."""
    k = 3 * h
    i0, i1, i2 = rand(seed, k + 1) % n, rand(seed, k + 2) % (n - 1), rand(seed, k + 3) % (n - 2)
    if mistake == "draws not distinct":
        return i0, i1, i2
    if i1 >= i0:
        i1 += 1
    lo, hi = min(i0, i1), max(i0, i1)
    if i2 >= lo:
        i2 += 1
    if i2 >= hi:
        i2 += 1
    return i0, i1, i2


# ------------------------------------------------------------------------------------------ the three-pair fit
def triad(p):
    """(F as 9 floats row-major with columns e1 e2 e3, c) of three points, or None: void."""
    d1 = [p[1][i] - p[0][i] for i in range(3)]
    d2 = [p[2][i] - p[0][i] for i in range(3)]
    cr = cross(d1, d2)
    n1, n2, nc = dot3(d1, d1), dot3(d2, d2), dot3(cr, cr)
    prod = n1 * n2
    if not prod > 0.0 or not nc >= MIN_SIN2 * prod:
        return None
    s1, s3 = math.sqrt(n1), math.sqrt(nc)
    e1 = [d1[i] / s1 for i in range(3)]
    e3 = [cr[i] / s3 for i in range(3)]
    e2 = cross(e3, e1)
    F = [0.0] * 9
    for i in range(3):
        F[3 * i], F[3 * i + 1], F[3 * i + 2] = e1[i], e2[i], e3[i]
    c = [((p[0][i] + p[1][i]) + p[2][i]) / 3.0 for i in range(3)]
    return F, c


def fit3(pq, pk, mistake=None):
    """(R as 9 floats, t) with p_k = R p_q + t, or None: void."""
    q, k = triad(pq), triad(pk)
    if q is None or k is None:
        if mistake != "void triads scored":
            return None
        return [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0], [0.0, 0.0, 0.0]
    (Fq, cq), (Fk, ck) = q, k
    R = [(Fk[3 * i] * Fq[3 * j] + Fk[3 * i + 1] * Fq[3 * j + 1]) + Fk[3 * i + 2] * Fq[3 * j + 2] for i in range(3) for j in range(3)]
    if mistake == "R transposed":
        R = [R[3 * j + i] for i in range(3) for j in range(3)]
    rc = mat_vec(R, cq)
    return R, [ck[i] - rc[i] for i in range(3)]


def hypothesis(cam, pairs, seed, h, mistake=None):
    """(R, t) of hypothesis h over the staged pairs, or None."""
    idx = draw(seed, h, len(pairs), mistake)
    pq, pk = [], []
    for s in idx:
        p = [float(v) for v in pairs[s]]
        pq.append(p[:3])
        d = triangulate(cam, p[3:])
        pk.append([p[3] * d, p[4] * d, d])
    return fit3(pq, pk, mistake)


# ------------------------------------------------------------------------------------------ error and score
def error2_all(cam, R, t, pairs, min_depth, mistake=None):
    """(valid bool[m], error2 float64[m]) of every staged pair under (R, t): element-wise numpy in the header's order."""
    R10, t10 = cam
    a0, a1, a2 = pairs[:, 0], pairs[:, 1], pairs[:, 2]
    with np.errstate(all="ignore"):
        p0 = [((R[3 * i] * a0 + R[3 * i + 1] * a1) + R[3 * i + 2] * a2) + t[i] for i in range(3)]
        p1 = [((R10[3 * i] * p0[0] + R10[3 * i + 1] * p0[1]) + R10[3 * i + 2] * p0[2]) + t10[i] for i in range(3)]
        valid = (p0[2] >= min_depth) & (p1[2] >= min_depth)
        r0, r1 = p0[0] / p0[2] - pairs[:, 3], p0[1] / p0[2] - pairs[:, 4]
        r2, r3 = p1[0] / p1[2] - pairs[:, 5], p1[1] / p1[2] - pairs[:, 6]
        e2 = (r0 * r0 + r1 * r1) if mistake == "cam1 residuals dropped" else ((r0 * r0 + r1 * r1) + r2 * r2) + r3 * r3
    return valid, e2


def error2_one(cam, R, t, pair, min_depth):
    """(valid, error2) of one pair, in Python floats: the definition."""
    R10, t10 = cam
    q = mat_vec(R, pair[:3])
    p0 = [q[i] + t[i] for i in range(3)]
    r1 = mat_vec(R10, p0)
    p1 = [r1[i] + t10[i] for i in range(3)]
    if not p0[2] >= min_depth or not p1[2] >= min_depth:
        return False, 0.0
    r = [p0[0] / p0[2] - pair[3], p0[1] / p0[2] - pair[4], p1[0] / p1[2] - pair[5], p1[1] / p1[2] - pair[6]]
    return True, ((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]) + r[3] * r[3]


def inlier_mask(cam, R, t, pairs, min_depth, max_error2, mistake=None):
    valid, e2 = error2_all(cam, R, t, pairs, min_depth, mistake)
    return valid & ((e2 <= max_error2) if mistake == "non-strict threshold" else (e2 < max_error2))


def key_of(count, h):
    return (1 << 32) | (count << 16) | (0xFFFF - h)


def key_h(key):
    return -1 if key == KEY_NONE else 0xFFFF - (key & 0xFFFF)


def key_count(key):
    return (key >> 16) & 0xFFFF


def merge(a, b):
    return max(a, b)


def score(cam, pairs, seed, K, min_depth, max_error2, mistake=None, h0=0):
    """The merged key of hypotheses h0 .. K - 1, and every hypothesis's count (-1: void)."""
    key, counts = KEY_NONE, []
    if len(pairs) < 3:
        return key, [-1] * (K - h0)
    for h in range(h0, K):
        hyp = hypothesis(cam, pairs, seed, h, mistake)
        if hyp is None:
            counts.append(-1)
            continue
        c = int(inlier_mask(cam, hyp[0], hyp[1], pairs, min_depth, max_error2, mistake).sum())
        counts.append(c)
        k = key_of(c, h)
        if mistake == "highest-h tie":
            key = k if key == KEY_NONE or key_count(k) >= key_count(key) else key
        else:
            key = merge(key, k)
    return key, counts


def score_slow(cam, pairs, seed, K, min_depth, max_error2):
    """The winner by a plain double loop over the definition: (best, count), (-1, 0) without one."""
    best, best_count = -1, -1
    if len(pairs) < 3:
        return -1, 0
    rows = [[float(v) for v in p] for p in pairs]
    for h in range(K):
        hyp = hypothesis(cam, pairs, seed, h)
        if hyp is None:
            continue
        c = 0
        for p in rows:
            ok, e2 = error2_one(cam, hyp[0], hyp[1], p, min_depth)
            c += 1 if ok and e2 < max_error2 else 0
        if c > best_count:
            best, best_count = h, c
    return (best, best_count) if best >= 0 else (-1, 0)


# ------------------------------------------------------------------------------------------ refinement
def chol6_solve(H, b):
    """x of H x = b by the unpivoted Cholesky of the header, or None: a pivot <= 0."""
    L = [0.0] * 36
    for j in range(6):
        s = H[6 * j + j]
        for k in range(j):
            s = s - L[6 * j + k] * L[6 * j + k]
        if not s > 0.0:
            return None
        ljj = math.sqrt(s)
        L[6 * j + j] = ljj
        for i in range(j + 1, 6):
            v = H[6 * i + j]
            for k in range(j):
                v = v - L[6 * i + k] * L[6 * j + k]
            L[6 * i + j] = v / ljj
    y, x = [0.0] * 6, [0.0] * 6
    for i in range(6):
        v = b[i]
        for k in range(i):
            v = v - L[6 * i + k] * y[k]
        y[i] = v / L[6 * i + i]
    for i in range(5, -1, -1):
        v = y[i]
        for k in range(i + 1, 6):
            v = v - L[6 * k + i] * x[k]
        x[i] = v / L[6 * i + i]
    return x


def normal_equations(cam, R, t, rows):
    """(H as 36 floats, g, sum of squared residuals) over the pairs `rows` in their order."""
    R10, t10 = cam
    H, g, S = [0.0] * 36, [0.0] * 6, 0.0
    for p in rows:
        q = mat_vec(R, p[:3])
        p0 = [q[i] + t[i] for i in range(3)]
        r1 = mat_vec(R10, p0)
        p1 = [r1[i] + t10[i] for i in range(3)]
        D0 = [[0.0, q[2], -q[1], 1.0, 0.0, 0.0], [-q[2], 0.0, q[0], 0.0, 1.0, 0.0], [q[1], -q[0], 0.0, 0.0, 0.0, 1.0]]
        D1 = [[(R10[3 * i] * D0[0][j] + R10[3 * i + 1] * D0[1][j]) + R10[3 * i + 2] * D0[2][j] for j in range(6)] for i in range(3)]
        u0, v0, u1, v1 = p0[0] / p0[2], p0[1] / p0[2], p1[0] / p1[2], p1[1] / p1[2]
        r = [u0 - p[3], v0 - p[4], u1 - p[5], v1 - p[6]]
        J = [[(D0[0][j] - u0 * D0[2][j]) / p0[2] for j in range(6)], [(D0[1][j] - v0 * D0[2][j]) / p0[2] for j in range(6)],
             [(D1[0][j] - u1 * D1[2][j]) / p1[2] for j in range(6)], [(D1[1][j] - v1 * D1[2][j]) / p1[2] for j in range(6)]]
        for k in range(4):
            for i in range(6):
                for j in range(i, 6):
                    H[6 * i + j] = H[6 * i + j] + J[k][i] * J[k][j]
                g[i] = g[i] + J[k][i] * r[k]
            S = S + r[k] * r[k]
    for i in range(6):
        for j in range(i):
            H[6 * i + j] = H[6 * j + i]
    return H, g, S


def small_rotation(th):
    vx, vy, vz = th[0] * 0.5, th[1] * 0.5, th[2] * 0.5
    nn = math.sqrt(((vx * vx + vy * vy) + vz * vz) + 1.0)
    x, y, z, w = vx / nn, vy / nn, vz / nn, 1.0 / nn
    return [1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y),
            2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x),
            2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y)]


def refine(cam, R, t, rows):
    """(R, t, info as 36 floats, rms), or None where a Cholesky pivot is <= 0 (or there is no pair)."""
    if not rows:
        return None
    R, t = list(R), list(t)
    for _ in range(REFINE_ITERS):
        H, g, S = normal_equations(cam, R, t, rows)
        dx = chol6_solve(H, [-v for v in g])
        if dx is None:
            return None
        dR = small_rotation(dx)
        R = [(dR[3 * i] * R[j] + dR[3 * i + 1] * R[3 + j]) + dR[3 * i + 2] * R[6 + j] for i in range(3) for j in range(3)]
        t = [t[i] + dx[3 + i] for i in range(3)]
    H, g, S = normal_equations(cam, R, t, rows)
    if chol6_solve(H, g) is None:
        return None
    return R, t, H, math.sqrt(S / (4.0 * float(len(rows))))


# ------------------------------------------------------------------------------------------ the whole job
def verify(query_obs, train_obs, T_cam1_cam0, max_error, usable=None, n_hypotheses=256, seed=0, min_depth=0.1, max_depth=40.0, mistake=None, do_refine=True):
    """What mskf_fe_verify returns: a dict of n_usable, n_inliers, best, status, inlier uint8[n], R (3, 3), t, info (6, 6), rms."""
    query_obs = np.asarray(query_obs, np.float64).reshape(-1, 4)
    train_obs = np.asarray(train_obs, np.float64).reshape(-1, 4)
    cam = cam_of(T_cam1_cam0)
    max_error2 = float(max_error) * float(max_error)
    pairs, orig = stage(cam, query_obs, train_obs, usable, float(min_depth), float(max_depth))
    out = dict(n_usable=len(pairs), n_inliers=0, best=-1, status=1, inlier=np.zeros(len(query_obs), np.uint8), R=np.eye(3), t=np.zeros(3), info=np.zeros((6, 6)), rms=0.0)
    key, _ = score(cam, pairs, int(seed), int(n_hypotheses), float(min_depth), max_error2, mistake)
    out["best"] = key_h(key)
    if out["best"] < 0:
        return out
    R, t = hypothesis(cam, pairs, int(seed), out["best"], mistake)
    mask = inlier_mask(cam, R, t, pairs, float(min_depth), max_error2, mistake)
    out["inlier"][orig[mask]] = 1
    out["n_inliers"], out["status"] = int(mask.sum()), 0
    if do_refine:
        ref = refine(cam, R, t, [[float(v) for v in p] for p in pairs[mask]])
        if ref is None:
            out["status"] = 2
        else:
            R, t, info, rms = ref
            out["info"], out["rms"] = np.array(info, np.float64).reshape(6, 6), rms
    out["R"], out["t"] = np.array(R, np.float64).reshape(3, 3), np.array(t, np.float64)
    return out
