"""Seeded inputs that drive the LK track kernel (k_track4) at its arithmetic and geometric edges, and helpers that say,
from the CPU oracle's per-point trace alone (oracle_py.lk_track_trace), what a set of inputs reaches.

A case is a dict: name, A, B (uint8 images: the template / search image of the temporal track), B1 (the cam1 image of
the stereo half: B shifted, so that the epipolar gate passes for a share of the points), pts (float32 n x 2), H (3 x 3
double, the Hpred of the temporal track; identity unless the case says otherwise).  The initial guess the oracle gets is
hpred_guess(H, pts): the device forms it the same way (predictFeatureTracking, image_processor.cpp:342-347).

tests/test_lk_cases.py holds the conditions that keep these sets from degenerating (no GPU); tests/test_gpu_lk_edges.py
runs them on the device.
"""
import math

import numpy as np

SIZES = [(64, 64), (65, 67), (129, 71), (333, 251), (255, 130), (1001, 99), (122, 509), (376, 240), (752, 480), (1280, 720)]
W11_FRACTIONS = [(64, 128), (2, 4096), (8192, 1), (128, 64), (1024, 8), (16, 512)]   # 14-bit (fa, fb) with w11 = -1
MARGIN = 48            # canvas margin: the largest shift of any case fits, so a shifted crop never wraps
MAX_POINTS = 1500      # per case: one track call of a default stream (its point capacity is 1624)
BORDER_VALUES_LO = (-16, -15, -14, -1, 0)       # template / guess corner values at the low side of a level
BORDER_VALUES_HI = (-16, -15, -2, -1, 0)        # ... relative to the level's width / height at the high side (-15: the
                                                # window's last column is the level's last; they keep that side trackable)
BORDER_FRACTIONS = (0.0, 0.59375)               # dyadic, so (v + 7 + f) * 2^l is exact in float32


def level_sizes(w, h):
    out = []
    for _ in range(4):
        out.append((w, h))
        w, h = (w + 1) // 2, (h + 1) // 2
    return out


def hpred_guess(H, pts):
    """k_track4's prediction: double, written order, rounded to float."""
    H = np.asarray(H, dtype=np.float64)
    px, py = pts[:, 0].astype(np.float64), pts[:, 1].astype(np.float64)
    X = H[0, 0] * px + H[0, 1] * py + H[0, 2] * 1.0
    Y = H[1, 0] * px + H[1, 1] * py + H[1, 2] * 1.0
    Z = H[2, 0] * px + H[2, 1] * py + H[2, 2] * 1.0
    return np.stack([(X / Z).astype(np.float32), (Y / Z).astype(np.float32)], 1)


def translation(tx, ty):
    return np.array([[1.0, 0.0, tx], [0.0, 1.0, ty], [0.0, 0.0, 1.0]])


def rotation_homography(w, h, roll_deg, tilt_x_deg, tilt_y_deg):
    """K R K^-1 of a camera with focal length 0.6 w and the principal point at the image centre."""
    f = 0.6 * w
    K = np.array([[f, 0.0, w / 2.0], [0.0, f, h / 2.0], [0.0, 0.0, 1.0]])
    a, b, c = (math.radians(v) for v in (roll_deg, tilt_x_deg, tilt_y_deg))
    Rz = np.array([[math.cos(a), -math.sin(a), 0], [math.sin(a), math.cos(a), 0], [0, 0, 1.0]])
    Rx = np.array([[1.0, 0, 0], [0, math.cos(b), -math.sin(b)], [0, math.sin(b), math.cos(b)]])
    Ry = np.array([[math.cos(c), 0, math.sin(c)], [0, 1.0, 0], [-math.sin(c), 0, math.cos(c)]])
    return K @ (Rz @ Rx @ Ry) @ np.linalg.inv(K)


# ---------------------------------------------------------------------------------------------- images
def crop(canvas, w, h, dx=0, dy=0):
    """The w x h view of the canvas moved by (dx, dy): a feature at p in crop(canvas) is at p + (dx, dy) here."""
    assert abs(dx) <= MARGIN and abs(dy) <= MARGIN
    return np.ascontiguousarray(canvas[MARGIN - dy:MARGIN - dy + h, MARGIN - dx:MARGIN - dx + w])


def block_canvas(w, h, block, seed):
    rng = np.random.default_rng(seed)
    H, W = h + 2 * MARGIN, w + 2 * MARGIN
    cells = rng.integers(0, 2, ((H + block - 1) // block, (W + block - 1) // block), dtype=np.uint8) * 255
    return np.ascontiguousarray(np.kron(cells, np.ones((block, block), np.uint8))[:H, :W])


def smooth_canvas(w, h, seed):
    """40 sinusoids of spatial frequency <= 0.12 rad/px: trackable over displacements of a few pixels at level 3."""
    rng = np.random.default_rng(seed)
    H, W = h + 2 * MARGIN, w + 2 * MARGIN
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    acc = np.zeros((H, W))
    for _ in range(40):
        fr, th, ph = rng.uniform(0.03, 0.12), rng.uniform(0, 2 * math.pi), rng.uniform(0, 2 * math.pi)
        acc += rng.uniform(0.5, 1.0) * np.sin(fr * (math.cos(th) * x + math.sin(th) * y) + ph)
    acc = (acc - acc.min()) / (acc.max() - acc.min())
    return np.ascontiguousarray(np.rint(acc * 255.0).astype(np.uint8))


def edge_canvas(w, h, seed, tile=12):
    """0/255 tiles of vertical, horizontal and diagonal step edges and of period-2 stripes.  The tiles are smaller than
    the window, so a window sees several patterns (a lone straight edge has no second gradient direction and is lost)."""
    rng = np.random.default_rng(seed)
    H, W = h + 2 * MARGIN, w + 2 * MARGIN
    yy, xx = np.mgrid[0:tile, 0:tile]
    pats = [xx >= tile // 2, yy >= tile // 2, xx + yy >= tile, xx >= yy, xx % 2 == 0, yy % 2 == 0, (xx + yy) % 2 == 0,
            xx < tile // 2, yy < tile // 2]
    out = np.zeros((H, W), np.uint8)
    for ty in range(0, H, tile):
        for tx in range(0, W, tile):
            p = pats[rng.integers(0, len(pats))].astype(np.uint8) * 255
            out[ty:ty + tile, tx:tx + tile] = p[:min(tile, H - ty), :min(tile, W - tx)]
    return out


def stripe_canvas(w, h, seed, vertical, band=8):
    """Period-4 0/255 stripes (0, 0, 255, 255) in bands of `band` pixels whose phase is random: at an integer template
    position every pixel inside a band has |I| = 4080 across the stripes, so the whole-window sums pass 2^31 (a window
    of 225 such pixels holds 3.7e9), and the phase steps between the bands give the other gradient direction."""
    rng = np.random.default_rng(seed)
    H, W = h + 2 * MARGIN, w + 2 * MARGIN
    if vertical:
        H, W = W, H
    phase = np.repeat(rng.integers(0, 4, (W + band - 1) // band), band)[:W]
    rows = np.arange(H)[:, None]
    out = ((((rows + phase[None, :]) % 4) >= 2) * 255).astype(np.uint8)
    return np.ascontiguousarray(out.T if vertical else out)


# ---------------------------------------------------------------------------------------------- points
def lattice(w, h, offset=0.37, pitch=7, max_points=MAX_POINTS):
    """Points on a square lattice with a sub-pixel offset; the pitch grows (from 7 px) until the count fits."""
    while True:
        xs = np.arange(pitch + offset, w - 1, pitch)
        ys = np.arange(pitch + offset, h - 1, pitch)
        if len(xs) * len(ys) <= max_points:
            break
        pitch += 1
    gx, gy = np.meshgrid(xs, ys)
    return np.stack([gx.ravel(), gy.ravel()], 1).astype(np.float32)


def _case(name, A, B, pts, H=None):
    return dict(name=name, A=A, B=B, pts=np.ascontiguousarray(pts, dtype=np.float32),
                H=np.eye(3) if H is None else np.asarray(H, dtype=np.float64))


_STEREO_SHIFT = {}


def stereo_shift(w, h, oracle):
    """Integer image motion cam0 -> cam1 that the stereo half can follow with oracle.euroc_calib(w, h): the median offset
    of its initial guess (the cam0 point turned into cam1; read off a flat pair, on which LK returns the guess
    unchanged) plus two pixels of disparity along the nearly horizontal epipolar lines."""
    if (w, h) not in _STEREO_SHIFT:
        from msckf_stereo_c_amd.ctypes_types import default_fe_cfg
        pts = lattice(w, h)
        flat = np.full((h, w), 128, np.uint8)
        guess, _ = oracle.stereo_match(oracle.euroc_calib(w, h), default_fe_cfg(), flat, flat, pts)
        med = np.median(guess - pts, 0)
        _STEREO_SHIFT[(w, h)] = (int(round(float(med[0]))) - 2, int(round(float(med[1]))))
    return _STEREO_SHIFT[(w, h)]


def shifted_replicate(img, sx, sy):
    """img moved by (sx, sy), the border replicated."""
    h, w = img.shape
    yi = np.clip(np.arange(h) - sy, 0, h - 1)
    xi = np.clip(np.arange(w) - sx, 0, w - 1)
    return np.ascontiguousarray(img[yi][:, xi])


def cases(set_name, w, h, oracle):
    """The cases of one set at one size, each with its cam1 image B1."""
    out = CASE_SETS[set_name](w, h)
    sx, sy = stereo_shift(w, h, oracle)
    for c in out:
        c["B1"] = shifted_replicate(c["B"], sx, sy)
    return out


# ---------------------------------------------------------------------------------------------- saturated
SAT_SHIFTS = [(0, 0), (1, 0), (3, 2), (0, 5)]


def saturated_cases(w, h, seed=1):
    """0/255 images: the magnitude bounds of the packed 16-bit arithmetic (|I| = 4080, |diff| = 8160, w11 = -1 on a 255
    pixel) and the largest lane / quad partial sums."""
    cases = []
    small = min(w, h) <= 72        # three or four pyramid-3 pixels of texture: 1 and 2 px blocks blur to nothing there
    for block in (1, 2, 3, 5, 8):
        if small and block < 3:
            shifts = [(0, 0), (1, 0)]
        else:
            shifts = SAT_SHIFTS
        canvas = block_canvas(w, h, block, seed * 100 + block)
        A = crop(canvas, w, h)
        for (dx, dy) in shifts:
            cases.append(_case("blocks%d_shift%d_%d" % (block, dx, dy), A, crop(canvas, w, h, dx, dy), lattice(w, h)))
    # step edges and period-2 stripes, templates at integer and at sub-pixel offsets
    canvas = edge_canvas(w, h, seed * 100 + 50)
    A = crop(canvas, w, h)
    for off in (0.0, 0.5, 0.37):
        cases.append(_case("edges_off%g" % off, A, crop(canvas, w, h, 1, 0), lattice(w, h, offset=off)))
    # extreme differences under a template that has gradient: the search image is the inverse, or half of it is
    # black / white (points near the half-plane's edge keep enough of the true image to be tracked)
    canvas = block_canvas(w, h, 5, seed * 100 + 60)
    A = crop(canvas, w, h)
    cases.append(_case("inverse", A, 255 - A, lattice(w, h)))
    for k, (val, vertical) in enumerate([(255, True), (0, True), (255, False), (0, False)]):
        B = crop(canvas, w, h, 1, 0).copy()
        if vertical:
            B[:, (w * (2 + k)) // 5:] = val
        else:
            B[(h * (k + 1)) // 5:, :] = val
        cases.append(_case("halfplane%d" % k, A, B, lattice(w, h)))
    # whole-window sums beyond 2^31 (the part of the row reduction the kernel carries in 64 bits): banded period-4 stripes,
    # templates at integer positions, the search image one pixel across the stripes (half the pixels differ by 8160)
    for vertical, band in ((False, 8), (True, 8)) + (((True, 16),) if small else ()):
        canvas = stripe_canvas(w, h, seed * 100 + 80 + vertical, vertical, band)
        A = crop(canvas, w, h)
        for (dx, dy) in ((0, 0), (1, 0) if vertical else (0, 1), (1, 1)):
            cases.append(_case("stripes4%s%d_shift%d_%d" % ("v" if vertical else "h", band, dx, dy), A, crop(canvas, w, h, dx, dy),
                               lattice(w, h, offset=0.0, pitch=3 if small else 7)))   # (small images: more windows to pick from)
    # the six (fa, fb) pairs whose fourth bilinear weight is -1, on an image full of 255-valued corners
    canvas = block_canvas(w, h, 3, seed * 100 + 70)
    pts = np.floor(lattice(w, h))
    for k, (fa, fb) in enumerate(W11_FRACTIONS):
        pts[k::6] += np.array([fa / 16384.0, fb / 16384.0], np.float32)
    cases.append(_case("w11_minus1", crop(canvas, w, h), crop(canvas, w, h, 1, 0), pts))
    return cases


# ---------------------------------------------------------------------------------------------- displaced
def _max_shift(w, h):
    """The displacement the smooth image is still tracked over: 30 px along x, 24 px along y (3.75 / 3 px at level 3), less
    where the image is too small to hold it."""
    return min(30, (w // 4) // 2 * 2), min(24, (h // 4) // 2 * 2)


def displaced_cases(w, h, seed=2):
    """Smooth images moved so far that the search window leaves the region staged at the start of a level (20 rows x 24
    bytes around the first window): the kernel has to re-stage inside its iteration loop."""
    cases = []
    canvas = smooth_canvas(w, h, seed * 100 + w + h)
    A = crop(canvas, w, h)
    sx, sy = _max_shift(w, h)
    rng = np.random.default_rng(seed)
    base = lattice(w, h)
    for name, (dx, dy) in (("px", (sx, 0)), ("mx", (-sx, 0)), ("py", (0, sy)), ("my", (0, -sy)), ("diag", (sx - 6, sy - 4)),
                           ("antidiag", (-(sx - 6), sy - 4))):
        cases.append(_case("shift_" + name, A, crop(canvas, w, h, dx, dy), base))
    # the displacement delivered by Hpred: the guess is the point turned by a few degrees about the optical axis (plus a
    # small tilt), the image itself moved a little, so the search travels from the turned guess back to the truth
    for k, (roll, dx, dy) in enumerate([(3.0, 4, -2), (-3.0, -3, 3), (2.0, 12, 8)]):
        Hm = rotation_homography(w, h, roll * min(1.0, 400.0 / max(w, h)), 0.4, -0.3)
        cases.append(_case("hpred%d" % k, A, crop(canvas, w, h, dx, dy), base, H=Hm))
    # B moved region by region (a 3 x 3 arrangement of regions with different displacements) and the points in a seeded
    # random order: the four consecutive points of a wavefront group sit in different regions and disagree about re-staging
    moves = [(0, sy), (sx, 0), (0, 0), (-sx, 0), (0, -sy), (2, 1), (sx - 6, sy - 4), (0, 0), (-(sx - 6), -(sy - 4))]
    for k in range(2):
        B = np.empty_like(A)
        order = rng.permutation(9)
        for ry in range(3):
            for rx in range(3):
                dx, dy = moves[order[ry * 3 + rx]]
                y0, y1, x0, x1 = (h * ry) // 3, (h * (ry + 1)) // 3, (w * rx) // 3, (w * (rx + 1)) // 3
                B[y0:y1, x0:x1] = crop(canvas, w, h, dx, dy)[y0:y1, x0:x1]
        cases.append(_case("regions%d" % k, A, B, base[rng.permutation(len(base))]))
    return cases


# ---------------------------------------------------------------------------------------------- border lattice
def border_values(n_l):
    """[(corner value, at the high side?)] of a level of n_l pixels."""
    return [(v, False) for v in BORDER_VALUES_LO] + [(n_l + v, True) for v in BORDER_VALUES_HI]


def border_coords(n):
    """Level-0 coordinates a whose window corner floorf(a * 2^-l - 7) takes each border value of each level l of an axis
    of n pixels, with two sub-pixel offsets each: [(a, level, value, high side?, offset index)]."""
    out = []
    for l in range(4):
        n_l = level_sizes(n, n)[l][0]
        for (v, hi) in border_values(n_l):
            for k, f in enumerate(BORDER_FRACTIONS):
                out.append(((v + 7 + f) * (1 << l), l, v, hi, k))
    return out


def border_points(w, h):
    """The lattice of all four sides and corners: (pts, side), side[i] = 0 left, 1 right, 2 top, 3 bottom, 4 corner."""
    xs, ys = border_coords(w), border_coords(h)
    inner_x = [int(w * 0.31) + 0.25, int(w * 0.68) + 0.5]        # dyadic like the lattice: a translated copy is exact
    inner_y = [int(h * 0.29) + 0.75, int(h * 0.71) + 0.125]
    pts, side = [], []
    for (a, _, _, hi, _) in xs:                  # left and right sides
        pts += [(a, y) for y in inner_y]
        side += [1 if hi else 0] * len(inner_y)
    for (a, _, _, hi, _) in ys:                  # top and bottom
        pts += [(x, a) for x in inner_x]
        side += [3 if hi else 2] * len(inner_x)
    for (a, la, _, _, ka) in xs:                 # the four corners: both axes at a border value of the same level
        for (b, lb, _, _, kb) in ys:
            if lb == la and ka == kb:
                pts.append((a, b))
                side.append(4)
    return np.array(pts, np.float32), np.array(side)


def border_cases(w, h, seed=3):
    """Points whose template corner, or whose initial guess' search corner, sits at the per-level in / out gates."""
    canvas = block_canvas(w, h, 4, seed * 100 + 1)
    A = crop(canvas, w, h)
    pts, _ = border_points(w, h)
    cases = [_case("border_template", A, crop(canvas, w, h, 1, 0), pts)]
    # the same lattice for the initial guess: the templates sit a translation away from it (most of them inside the
    # image), Hpred carries them onto the lattice, and the image moves the same way
    tx, ty = min(16, w // 4), min(12, h // 4)
    for name, (dx, dy) in (("left", (-tx, 0)), ("right", (tx, 0)), ("up", (0, -ty)), ("down", (0, ty))):
        src = (pts.astype(np.float64) - np.array([dx, dy], np.float64)).astype(np.float32)
        cases.append(_case("border_guess_" + name, A, crop(canvas, w, h, dx, dy), src, H=translation(dx, dy)))
    return cases


def sizes_cases(w, h, seed=4):
    """A moderate-contrast textured pair with a small motion: the plain geometry check of every size."""
    canvas = (smooth_canvas(w, h, seed * 100 + 7).astype(np.int32) * 3 // 4 + block_canvas(w, h, 4, seed * 100 + 8) // 8).astype(np.uint8)
    return [_case("plain", crop(canvas, w, h), crop(canvas, w, h, 2, -1), lattice(w, h))]


CASE_SETS = dict(saturated=saturated_cases, displaced=displaced_cases, border=border_cases, sizes=sizes_cases)


# ---------------------------------------------------------------------------------------------- a track result against the oracle
def bits(a):
    return np.ascontiguousarray(a).view(np.uint32) if a.dtype == np.float32 else a


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def check_track(got, oracle, calib, fe, c, do_temporal, tag):
    """One track result (out0, out1, und0, und1, status of the points of case c) against the oracle: LK, then the bounds gate,
    then oracle.stereo_match and oracle.undistort; survivors bit-exact in every output, the rest zero.  Returns the numbers of
    tracked points and of stereo inliers."""
    h, w = c["B"].shape
    pts = c["pts"]
    n = len(pts)
    K0, D0 = np.array(calib.cam0_intrinsics), np.array(calib.cam0_distortion)
    K1, D1 = np.array(calib.cam1_intrinsics), np.array(calib.cam1_distortion)
    if do_temporal:
        ref_b, ref_st = oracle.lk_track(c["A"], c["B"], pts, hpred_guess(c["H"], pts))
        ok = ref_st.astype(bool)
        ok &= ~((ref_b[:, 1] < 0) | (ref_b[:, 1] > h - 1) | (ref_b[:, 0] < 0) | (ref_b[:, 0] > w - 1))
    else:
        ref_b, ok = pts, np.ones(n, bool)
    assert np.array_equal((got["status"] & 1).astype(bool), ok), tag
    assert same(got["out0"][ok], ref_b[ok]), tag
    # a point that fails the temporal half: status 0 and out1 = und0 = und1 = 0 (include/mskf_hip.h)
    lost = ~ok
    assert (got["status"][lost] == 0).all(), tag
    for k in ("out1", "und0", "und1"):
        assert (bits(got[k][lost]) == 0).all(), (tag, k)
    n_in = 0
    if ok.any():
        tracked = np.ascontiguousarray(ref_b[ok])
        ref_c1, ref_in = oracle.stereo_match(calib, fe, c["B"], c["B1"], tracked)
        assert np.array_equal((got["status"][ok] >> 1) & 1, ref_in), tag
        assert same(got["out1"][ok], ref_c1), tag
        assert same(got["und0"][ok], oracle.undistort(K0, D0, tracked, model=calib.cam0_model)), tag
        assert same(got["und1"][ok], oracle.undistort(K1, D1, ref_c1, model=calib.cam1_model)), tag
        n_in = int(ref_in.sum())
    return int(ok.sum()), n_in


# ---------------------------------------------------------------------------------------------- what the trace says
def in_image(pts, w, h):
    return (pts[:, 0] >= 0) & (pts[:, 0] <= w - 1) & (pts[:, 1] >= 0) & (pts[:, 1] <= h - 1)


def forced_restage(trace):
    """Per point and level: must the kernel re-stage its search region at that level?  Only the kernel's documented rule
    is used (region origin bx0 = (inx0 - 2) & ~3, by0 = iny0 - 2; the window offset may be ox 0..8, oy 0..4), on the
    extremes of the search corner over the iterations that ran: a sufficient condition, not a necessary one.
    Returns bool arrays [n, 4] for the directions +x, -x, +y, -y."""
    L = trace["lvl"]
    ran = L["iters"] > 0
    bx0 = (L["inx0"] - 2) & ~3
    by0 = L["iny0"] - 2
    px = ran & (L["inx_max"] - bx0 > 8)
    mx = ran & (L["inx_min"] - bx0 < 0)
    py = ran & (L["iny_max"] - by0 > 4)
    my = ran & (L["iny_min"] - by0 < 0)
    return px, mx, py, my
