"""Restatement of the L-level pyramidal LK of the opt-in deeper pyramids ("Deeper LK pyramids"; l4_track<true> on
the device), written from the contract: the arithmetic of oracle/o_image.cpp::lk_track_point_trace with LK_LEVELS replaced by L,
over chains of oracle_py.pyr_down.

    pyramid     level l is pyr_down of level l - 1, ((w + 1) / 2, (h + 1) / 2), for every l < L.
    LK          for l = L - 1 .. 0: sc = 2^-l; the guess is scaled once at the top level and doubled per level; a level whose template
                corner is outside [-15, size) or whose minEig / determinant test fails passes the guess on unchanged; status 0 is set
                by level 0 only (bounds, minEig, or the search corner leaving the level during the iterations).
    fixed point 14-bit bilinear weights (w11 = 2^14 - the others), samples (s + 256) >> 9, Scharr (3, 10, 3) gradients (s + 16) >> 5,
                integer sums, * 2^-20 in double, the 2 x 2 solve in double rounded to float32, float32 positions.

At L = 4 it gives the bits of oracle_py.lk_track; at L = 8 those of two chained oracle runs (tests/test_deep_lk_reference.py).
Also here: the validity rule restated (max_levels), the stereo match and the frame's track steps with the LK replaced (stereo_match,
DeepOracle: the `oracle` argument of frame_cases.track_reference / the LK of fb_reference), and the scenes of the capture-range
tests.  `mutate` plants one deliberate mistake (MUTATIONS)."""
import numpy as np

import lk_cases as LC

WIN, HALF, ITERS = 15, 7, 30
MIN_LEVELS, MAX_LEVELS = 4, 8
MUTATIONS = [
    "guess_not_doubled",   # the guess is passed down a level without the factor 2
    "status_from_top",     # a failing top level sets status 0, as level 0 does
    "sc_wrong_level",      # sc = 2^-(l + 1) above level 3 (the scale of the wrong level)
]
F32 = np.float32


def level_sizes(w, h, levels):
    out = []
    for _ in range(levels):
        out.append((w, h))
        w, h = (w + 1) // 2, (h + 1) // 2
    return out


def max_levels(w, h):
    """The largest L in 4 .. 8 whose level L - 1 has both sides >= 15 (4 is always allowed: it is what runs without the option)."""
    L = MIN_LEVELS
    while L < MAX_LEVELS and min(level_sizes(w, h, L + 1)[L]) >= WIN:
        L += 1
    return L


def pyramid(img, levels):
    from oracle import oracle_py
    pyr = [np.ascontiguousarray(img)]
    for _ in range(levels - 1):
        pyr.append(oracle_py.pyr_down(pyr[-1]))
    return pyr


def _weights(fa, fb):
    qa, qb = int(np.rint(F32(fa) * F32(16384.0))), int(np.rint(F32(fb) * F32(16384.0)))
    w00 = ((16384 - qa) * (16384 - qb) + 8192) >> 14
    w01 = (qa * (16384 - qb) + 8192) >> 14
    w10 = ((16384 - qa) * qb + 8192) >> 14
    return w00, w01, w10, 16384 - w00 - w01 - w10


def _samples(img, x0, y0, n, w):
    """(n x n) samples at integer corners (x0 + i, y0 + j), pixels outside the image replicated from the border."""
    h_, w_ = img.shape
    ys = np.clip(np.arange(y0, y0 + n + 1), 0, h_ - 1)
    xs = np.clip(np.arange(x0, x0 + n + 1), 0, w_ - 1)
    p = img[ys][:, xs].astype(np.int64)
    s = p[:-1, :-1] * w[0] + p[:-1, 1:] * w[1] + p[1:, :-1] * w[2] + p[1:, 1:] * w[3]
    return (s + 256) >> 9


def _track_point(pyrA, pyrB, ax, ay, bx, by, levels, mutate):
    status = 1
    ncx = ncy = F32(0)
    top = levels - 1
    for l in range(top, -1, -1):
        A, B = pyrA[l], pyrB[l]
        sc = F32(1.0) / F32(1 << (l + 1 if mutate == "sc_wrong_level" and l >= 4 else l))
        pwx, pwy = F32(ax * sc - F32(HALF)), F32(ay * sc - F32(HALF))
        if l == top:
            ncx, ncy = F32(bx * sc), F32(by * sc)
        elif mutate != "guess_not_doubled":
            ncx, ncy = F32(ncx * F32(2)), F32(ncy * F32(2))
        ipx, ipy = int(np.floor(pwx)), int(np.floor(pwy))
        lowest = l == 0 or (mutate == "status_from_top" and l == top)
        if ipx < -WIN or ipx >= A.shape[1] or ipy < -WIN or ipy >= A.shape[0]:
            if lowest:
                status = 0
            continue
        P = _samples(A, ipx - 1, ipy - 1, 17, _weights(F32(pwx - F32(ipx)), F32(pwy - F32(ipy))))      # P[j + 1][i + 1]
        sx = 3 * (P[:-2, 2:] - P[:-2, :-2]) + 10 * (P[1:-1, 2:] - P[1:-1, :-2]) + 3 * (P[2:, 2:] - P[2:, :-2])
        sy = 3 * (P[2:, :-2] - P[:-2, :-2]) + 10 * (P[2:, 1:-1] - P[:-2, 1:-1]) + 3 * (P[2:, 2:] - P[:-2, 2:])
        Ix, Iy = (sx + 16) >> 5, (sy + 16) >> 5
        T = P[1:-1, 1:-1]
        scale = 1.0 / (1 << 20)
        a11, a12, a22 = float(int((Ix * Ix).sum())) * scale, float(int((Ix * Iy).sum())) * scale, float(int((Iy * Iy).sum())) * scale
        D = a11 * a22 - a12 * a12
        dd = a11 - a22
        min_eig = (a22 + a11 - np.sqrt(np.float64(dd * dd + 4.0 * a12 * a12))) / (2.0 * WIN * WIN)
        if min_eig < 1e-4 or D < float(np.finfo(np.float32).eps):
            if lowest:
                status = 0
            continue
        D = 1.0 / D
        wx, wy = F32(ncx - F32(HALF)), F32(ncy - F32(HALF))
        pdx = pdy = F32(0)
        for it in range(ITERS):
            inx, iny = int(np.floor(wx)), int(np.floor(wy))
            if inx < -WIN or inx >= B.shape[1] or iny < -WIN or iny >= B.shape[0]:
                if lowest:
                    status = 0
                break
            diff = _samples(B, inx, iny, 15, _weights(F32(wx - F32(inx)), F32(wy - F32(iny)))) - T
            db1, db2 = float(int((diff * Ix).sum())) * scale, float(int((diff * Iy).sum())) * scale
            dx, dy = F32((a12 * db2 - a22 * db1) * D), F32((a12 * db1 - a11 * db2) * D)
            wx, wy = F32(wx + dx), F32(wy + dy)
            if float(dx) * float(dx) + float(dy) * float(dy) <= 0.01 * 0.01:
                break
            if it > 0 and abs(F32(dx + pdx)) < F32(0.01) and abs(F32(dy + pdy)) < F32(0.01):
                wx, wy = F32(wx - F32(dx * F32(0.5))), F32(wy - F32(dy * F32(0.5)))
                break
            pdx, pdy = dx, dy
        ncx, ncy = F32(wx + F32(HALF)), F32(wy + F32(HALF))
    return ncx, ncy, status


def lk_track_pyr(pyrA, pyrB, ptsA, guess, levels, mutate=None):
    a = np.ascontiguousarray(ptsA, dtype=np.float32).reshape(-1, 2)
    b = np.ascontiguousarray(guess, dtype=np.float32).reshape(-1, 2).copy()
    st = np.zeros(len(a), np.uint8)
    with np.errstate(over="ignore", invalid="ignore"):
        for i in range(len(a)):
            b[i, 0], b[i, 1], st[i] = _track_point(pyrA, pyrB, a[i, 0], a[i, 1], b[i, 0], b[i, 1], levels, mutate)
    return b, st


_PYR = {}


def _pyr_of(img, levels):
    """Pyramids are cached per image object (the tests track many point sets over few images)."""
    key = (id(img), levels)
    if key not in _PYR or _PYR[key][0] is not img:
        if len(_PYR) > 64:
            _PYR.clear()
        _PYR[key] = (img, pyramid(img, levels))
    return _PYR[key][1]


def lk_track(imgA, imgB, ptsA, guess, levels=4, mutate=None):
    """(positions float32 [n, 2], status uint8 [n]) of the L-level track: oracle_py.lk_track's signature plus the depth."""
    return lk_track_pyr(_pyr_of(imgA, levels), _pyr_of(imgB, levels), ptsA, guess, levels, mutate)


# ---------------------------------------------------------------------------------------------- the stereo match with this LK
def _m3(a, b):
    r = np.zeros((3, 3))
    for i in range(3):
        for j in range(3):
            s = 0.0
            for k in range(3):
                s += a[i, k] * b[k, j]
            r[i, j] = s
    return r


def _mv(a, b):
    return np.array([a[i, 0] * b[0] + a[i, 1] * b[1] + a[i, 2] * b[2] for i in range(3)])


def essential(calib):
    """E = [t]x R_cam0_cam1 and the epipolar threshold's pixel unit, by the oracle's statements (o_frontend.cpp: loadParameters,
    stereoMatch), double operation for double operation."""
    T0 = np.array(list(calib.T_cam0_imu), np.float64).reshape(4, 4)
    T10 = np.array(list(calib.T_cam1_cam0), np.float64).reshape(4, 4)
    R_cam0_imu = T0[:3, :3].T.copy()
    t_cam0_imu = -_mv(R_cam0_imu, T0[:3, 3])
    R1, t1 = _m3(T10[:3, :3], T0[:3, :3]), _mv(T10[:3, :3], T0[:3, 3]) + T10[:3, 3]
    R_cam1_imu = R1.T.copy()
    t_cam1_imu = -_mv(R_cam1_imu, t1)
    R01 = _m3(R_cam1_imu.T, R_cam0_imu)
    t = _mv(R_cam1_imu.T, t_cam0_imu - t_cam1_imu)
    S = np.array([[0.0, -t[2], t[1]], [t[2], 0.0, -t[0]], [-t[1], t[0], 0.0]])
    K0, K1 = list(calib.cam0_intrinsics), list(calib.cam1_intrinsics)
    return _m3(S, R01), 4.0 / (K0[0] + K0[1] + K1[0] + K1[1])


def stereo_match(oracle, calib, fe, cam0, cam1, pts0, levels=4, mutate=None):
    """oracle.stereo_match with its LK replaced: the rotation-only guess (read off a flat pair, on which the oracle's LK returns
    the guess unchanged), the L-level track, the bounds gate, the epipolar gate on the undistorted points."""
    p0 = np.ascontiguousarray(pts0, dtype=np.float32).reshape(-1, 2)
    if not len(p0):
        return p0.copy(), np.zeros(0, np.uint8)
    flat = np.full(cam0.shape, 128, np.uint8)
    guess, _ = oracle.stereo_match(calib, fe, flat, flat, p0)
    c1, st = lk_track(cam0, cam1, p0, guess, levels, mutate)
    h, w = cam1.shape
    inl = st.astype(bool) & ~((c1[:, 1] < 0) | (c1[:, 1] > h - 1) | (c1[:, 0] < 0) | (c1[:, 0] > w - 1))
    u0 = oracle.undistort(np.array(calib.cam0_intrinsics), np.array(calib.cam0_distortion), p0, model=calib.cam0_model).astype(np.float64)
    u1 = oracle.undistort(np.array(calib.cam1_intrinsics), np.array(calib.cam1_distortion), c1, model=calib.cam1_model).astype(np.float64)
    E, unit = essential(calib)
    x0, y0, x1, y1 = u0[:, 0], u0[:, 1], u1[:, 0], u1[:, 1]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        l0 = (E[0, 0] * x0 + E[0, 1] * y0) + E[0, 2]
        l1 = (E[1, 0] * x0 + E[1, 1] * y0) + E[1, 2]
        l2 = (E[2, 0] * x0 + E[2, 1] * y0) + E[2, 2]
        err = np.abs((x1 * l0 + y1 * l1) + l2) / np.sqrt(l0 * l0 + l1 * l1)
        inl &= ~(err > fe.stereo_threshold * unit)
    return c1, inl.astype(np.uint8)


class DeepOracle:
    """oracle_py with lk_track and stereo_match at `levels`: what frame_cases.track_reference / stereo_reference take as `oracle`."""

    def __init__(self, oracle, levels, mutate=None):
        self._o, self.levels, self.mutate = oracle, levels, mutate

    def __getattr__(self, name):
        return getattr(self._o, name)

    def lk_track(self, imgA, imgB, ptsA, guess):
        return lk_track(imgA, imgB, ptsA, guess, self.levels, self.mutate)

    def stereo_match(self, calib, fe, cam0, cam1, pts0):
        return stereo_match(self._o, calib, fe, cam0, cam1, pts0, self.levels, self.mutate)


# ---------------------------------------------------------------------------------------------- the capture-range scenes
SCENE_SEED = 7
_SCENES = {}


def scene(w, h, shift, reach=64):
    """(A, B, pts): the smooth canvas of lk_cases (seed 7) and its copy moved `shift` pixels along x (B = crop of a canvas wide
    enough for the shift), lattice points whose truth lies inside B with a window's margin for every shift up to `reach`, so
    that the scenes of different shifts carry the same points."""
    assert 0 <= shift <= reach <= 64
    key = (w, h, shift, reach)
    if key not in _SCENES:
        ck = ("canvas", w, h)
        if ck not in _SCENES:
            _SCENES[ck] = LC.smooth_canvas(w + 128, h, SCENE_SEED)       # 64 more columns of margin on either side
        canvas = _SCENES[ck]
        m = LC.MARGIN + 64
        A = np.ascontiguousarray(canvas[LC.MARGIN:LC.MARGIN + h, m:m + w])
        B = np.ascontiguousarray(canvas[LC.MARGIN:LC.MARGIN + h, m - shift:m - shift + w])
        pts = LC.lattice(w, h, pitch=max(w, h) // 8)
        keep = (pts[:, 0] + reach < w - 24) & (pts[:, 0] > 24) & (pts[:, 1] > 24) & (pts[:, 1] < h - 24)
        for a in (A, B):
            a.setflags(write=False)
        _SCENES[key] = (A, B, np.ascontiguousarray(pts[keep]))
    return _SCENES[key]


def tracked(b, st, pts, shift, tol=0.5):
    """bool per point: status != 0 and within `tol` pixels of the truth pts + (shift, 0)."""
    d = b.astype(np.float64) - (pts.astype(np.float64) + np.array([shift, 0.0]))
    return (st != 0) & (np.hypot(d[:, 0], d[:, 1]) <= tol)
