"""Plain numpy restatement of the equalisation contract ("Equalisation"), written from the contract's text and
not from csrc/hip/fe_equalize.h: global histogram equalisation (`equalize_hist`) and CLAHE (`clahe`) of an 8-bit image.

Float arithmetic is numpy float32, one operation per step (numpy never contracts a multiply and an add).  `mutate` switches
on one deliberate mistake, for the tests that show the comparison set can see it:
    "truncate"        sat8 truncates instead of rounding half to even
    "residual_first"  the residual of the redistribution goes to the first `residual` bins
    "clamp_first"     the tile indices are clamped before the interpolation weight is formed
"""
import numpy as np

F = np.float32
MUTATIONS = ("truncate", "residual_first", "clamp_first")


def sat8(x, mutate=None):
    x = np.asarray(x, dtype=F)
    r = np.trunc(x) if mutate == "truncate" else np.rint(x)        # np.rint: round half to even
    return np.clip(r, 0, 255).astype(np.uint8)


def equalize_hist(img, mutate=None):
    img = np.ascontiguousarray(img, dtype=np.uint8)
    total = img.size
    hist = np.bincount(img.reshape(-1), minlength=256).astype(np.int64)
    i0 = int(np.nonzero(hist)[0][0])
    if hist[i0] == total:
        return img.copy()
    scale = F(255.0) / F(total - hist[i0])
    lut = np.zeros(256, np.uint8)
    s = 0
    for i in range(i0 + 1, 256):
        s += int(hist[i])
        lut[i] = sat8(F(s) * scale, mutate)
    return lut[img]


def tile_geometry(w, h, tiles_x, tiles_y):
    """(tile width, tile height) of the virtually extended image."""
    if w % tiles_x == 0 and h % tiles_y == 0:
        ew, eh = w, h
    else:
        ew, eh = w + (tiles_x - w % tiles_x), h + (tiles_y - h % tiles_y)
    return ew // tiles_x, eh // tiles_y


def reflect_col(c, w):
    """BORDER_REFLECT_101."""
    if w == 1:
        return 0
    while c < 0 or c >= w:
        c = -c if c < 0 else 2 * (w - 1) - c
    return c


def reflect_row(r, h):
    """REFLECT_101 up to 2h - 2, folding again beyond it (the contract's row rule)."""
    if r < h:
        return r
    if h == 1:
        return 0
    return (h - 1) - ((r - (h - 1)) % (h - 1))


def clip_of(clip_limit, T):
    """None: no clip."""
    if not clip_limit > 0:
        return None
    return max(int(float(clip_limit) * T / 256.0), 1)


def clip_and_redistribute(hist, clip, mutate=None):
    """-> (new histogram, clipped).  hist: 256 counts."""
    hist = [int(v) for v in hist]
    if clip is None:
        return hist, 0
    clipped = sum(max(v - clip, 0) for v in hist)
    hist = [min(v, clip) for v in hist]
    batch, residual = clipped // 256, clipped % 256
    hist = [v + batch for v in hist]
    if residual:
        if mutate == "residual_first":
            for i in range(residual):
                hist[i] += 1
        else:
            step = max(256 // residual, 1)
            i = 0
            while i < 256 and residual > 0:
                hist[i] += 1
                i += step
                residual -= 1
    return hist, clipped


def tile_lut(hist, T, clip, mutate=None):
    hist, _ = clip_and_redistribute(hist, clip, mutate)
    scale = F(255.0) / F(T)
    cum = np.cumsum(np.asarray(hist, dtype=np.int64))
    return sat8(cum.astype(F) * scale, mutate)


def _axis(n, t, n_tiles, mutate=None):
    """Per position 0 .. n - 1: first tile, second tile (both clamped), weight of the second, weight of the first."""
    inv = F(1.0) / F(t)
    f = np.arange(n, dtype=F) * inv - F(0.5)
    t1 = np.floor(f).astype(np.int64)
    t2 = t1 + 1
    if mutate == "clamp_first":
        t1 = np.maximum(t1, 0)
        t2 = np.minimum(t2, n_tiles - 1)
    a = f - t1.astype(F)
    a1 = F(1.0) - a
    t1 = np.maximum(t1, 0)
    t2 = np.minimum(t2, n_tiles - 1)
    return t1, t2, a.astype(F), a1.astype(F)


def clahe_luts(img, tiles_x, tiles_y, clip_limit, mutate=None):
    img = np.ascontiguousarray(img, dtype=np.uint8)
    h, w = img.shape
    tw, th = tile_geometry(w, h, tiles_x, tiles_y)
    rows = np.array([reflect_row(r, h) for r in range(th * tiles_y)])
    cols = np.array([reflect_col(c, w) for c in range(tw * tiles_x)])
    ext = img[np.ix_(rows, cols)]
    T = tw * th
    clip = clip_of(clip_limit, T)
    luts = np.zeros((tiles_y, tiles_x, 256), np.uint8)
    for ty in range(tiles_y):
        for tx in range(tiles_x):
            tile = ext[ty * th:(ty + 1) * th, tx * tw:(tx + 1) * tw]
            luts[ty, tx] = tile_lut(np.bincount(tile.reshape(-1), minlength=256), T, clip, mutate)
    return luts


def clahe(img, tiles_x=8, tiles_y=8, clip_limit=40.0, mutate=None):
    img = np.ascontiguousarray(img, dtype=np.uint8)
    h, w = img.shape
    tw, th = tile_geometry(w, h, tiles_x, tiles_y)
    luts = clahe_luts(img, tiles_x, tiles_y, clip_limit, mutate)
    y1, y2, ya, ya1 = _axis(h, th, tiles_y, mutate)
    x1, x2, xa, xa1 = _axis(w, tw, tiles_x, mutate)
    Y1, Y2, X1, X2 = y1[:, None], y2[:, None], x1[None, :], x2[None, :]
    l11 = luts[Y1, X1, img].astype(F)
    l12 = luts[Y1, X2, img].astype(F)
    l21 = luts[Y2, X1, img].astype(F)
    l22 = luts[Y2, X2, img].astype(F)
    XA, XA1, YA, YA1 = xa[None, :], xa1[None, :], ya[:, None], ya1[:, None]
    top = l11 * XA1 + l12 * XA
    bot = l21 * XA1 + l22 * XA
    return sat8(top * YA1 + bot * YA, mutate)


def equalize(img, mode, tiles=(8, 8), clip_limit=40.0, mutate=None):
    """mode 0 / "off", 1 / "hist", 2 / "clahe"."""
    mode = {"off": 0, "hist": 1, "clahe": 2}.get(mode, mode)
    if mode == 0:
        return np.ascontiguousarray(img, dtype=np.uint8).copy()
    if mode == 1:
        return equalize_hist(img, mutate)
    return clahe(img, tiles[0], tiles[1], clip_limit, mutate)


# ---- the image set the harness, the mutations and the GPU tests share
def structured_images(w, h, seed=0):
    """name -> h x w uint8: random, low-contrast random, flat, step, 1-pixel checkerboard, 0 / 255 saturated, ramp."""
    rng = np.random.default_rng(seed * 7919 + w * 31 + h)
    yy, xx = np.mgrid[0:h, 0:w]
    out = {
        "random": rng.integers(0, 256, (h, w)).astype(np.uint8),
        "lowcontrast": (96 + rng.integers(0, 32, (h, w))).astype(np.uint8),
        "flat": np.full((h, w), 77, np.uint8),
        "step": np.where(xx < w // 2, 40, 200).astype(np.uint8),
        "checker": np.where((xx + yy) % 2 == 0, 13, 240).astype(np.uint8),
        "saturated": np.where(rng.random((h, w)) < 0.5, 0, 255).astype(np.uint8),
        "ramp": ((xx * 3 + yy * 5) % 256).astype(np.uint8),
    }
    # a smooth scene with a few outliers: most bins of a tile empty, some far over any clip
    blob = (120 + 30 * np.sin(xx / 9.0) * np.cos(yy / 7.0)).astype(np.uint8)
    blob[rng.random((h, w)) < 0.02] = 255
    out["scene"] = blob
    return out
