"""Numpy restatement of the input pixel formats of a stream ("Input pixel formats"), written from the list there
and not from csrc/hip/fe_pixfmt.h.  Integer arithmetic throughout: device, header-on-CPU and this file agree bit for bit.

    convert(raw, fmt, shift)      raw image in the format's dtype and shape -> (h, w) uint8, the stream's level 0

raw: gray8 and the Bayer mosaics (h, w) uint8; gray16 (h, w) uint16; rgb8 / bgr8 (h, w, 3) uint8; rgba8 / bgra8 (h, w, 4) uint8.
`mutate` plants one deliberate mistake (MUTATIONS), for the tests that show the comparison set would see it."""
import ctypes as C

import numpy as np

FORMATS = {"gray8": 0, "gray16": 1, "rgb8": 2, "bgr8": 3, "rgba8": 4, "bgra8": 5,
           "bayer_rggb8": 6, "bayer_grbg8": 7, "bayer_gbrg8": 8, "bayer_bggr8": 9}
NAMES = {v: k for k, v in FORMATS.items()}
BPP = {"gray8": 1, "gray16": 2, "rgb8": 3, "bgr8": 3, "rgba8": 4, "bgra8": 4,
       "bayer_rggb8": 1, "bayer_grbg8": 1, "bayer_gbrg8": 1, "bayer_bggr8": 1}
BAYER = [n for n in FORMATS if n.startswith("bayer_")]
MUTATIONS = ["swap_rb", "clamp", "no_round"]


class PxJob(C.Structure):
    """PxJob of csrc/hip/fe_pixfmt.h: one image of the conversion kernel, as the GPU tests hand it to fe_launch_px_convert.
    tests/test_pixel_format_reference.py compares it with the header's own size and field offsets (px_job_layout)."""
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("pitch", C.c_longlong),
                ("w", C.c_int32), ("h", C.c_int32), ("format", C.c_int32), ("shift", C.c_int32)]


def name_of(fmt):
    return NAMES[fmt] if not isinstance(fmt, str) else fmt


def luma(r, g, b, mutate=None):
    """Y = (9798 R + 19235 G + 3735 B + 16384) >> 15 on integer arrays."""
    r, g, b = (np.asarray(v).astype(np.int64) for v in (r, g, b))
    wr, wb = (3735, 9798) if mutate == "swap_rb" else (9798, 3735)
    return (wr * r + 19235 * g + wb * b + (0 if mutate == "no_round" else 16384)) >> 15


def gray16(v, shift):
    return np.minimum(np.asarray(v).astype(np.int64) >> shift, 255)


def bayer_rgb(p, fmt, mutate=None):
    """Bilinear (R, G, B) planes of the mosaic p; out-of-image neighbours by REFLECT_101."""
    letters = name_of(fmt)[len("bayer_"):len("bayer_") + 4].upper()
    p = np.asarray(p).astype(np.int64)
    h, w = p.shape
    assert w >= 2 and h >= 2
    q = np.pad(p, 1, mode="edge" if mutate == "clamp" else "reflect")      # numpy's "reflect" is REFLECT_101
    c = q[1:-1, 1:-1]
    l, r, u, d = q[1:-1, :-2], q[1:-1, 2:], q[:-2, 1:-1], q[2:, 1:-1]
    ul, ur, dl, dr = q[:-2, :-2], q[:-2, 2:], q[2:, :-2], q[2:, 2:]
    cross, diag = (l + r + u + d + 2) >> 2, (ul + ur + dl + dr + 2) >> 2
    hor, ver = (l + r + 1) >> 1, (u + d + 1) >> 1
    yy, xx = np.mgrid[0:h, 0:w]
    site = np.array(list(letters))[(yy & 1) * 2 + (xx & 1)]                   # the colour each site samples
    row_nb = np.array(list(letters))[(yy & 1) * 2 + ((xx & 1) ^ 1)]           # the colour of its row neighbours
    out = {}
    for col, opp in (("R", "B"), ("B", "R")):
        plane = np.where(site == col, c, 0)
        plane = np.where(site == opp, diag, plane)
        plane = np.where((site == "G") & (row_nb == col), hor, plane)
        plane = np.where((site == "G") & (row_nb != col), ver, plane)
        out[col] = plane
    out["G"] = np.where(site == "G", c, cross)
    return out["R"], out["G"], out["B"]


def convert(raw, fmt, shift=0, mutate=None):
    name = name_of(fmt)
    raw = np.asarray(raw)
    if name == "gray8":
        assert raw.dtype == np.uint8 and raw.ndim == 2
        return raw.copy()
    if name == "gray16":
        assert raw.dtype == np.uint16 and raw.ndim == 2
        return gray16(raw, shift).astype(np.uint8)
    assert raw.dtype == np.uint8
    if name in BAYER:
        return luma(*bayer_rgb(raw, name, mutate), mutate=mutate).astype(np.uint8)
    assert raw.ndim == 3 and raw.shape[2] == BPP[name]
    r, b = (raw[..., 0], raw[..., 2]) if name in ("rgb8", "rgba8") else (raw[..., 2], raw[..., 0])
    return luma(r, raw[..., 1], b, mutate=mutate).astype(np.uint8)


def raw_bytes(raw, fmt, pad=0, fill=0xEE):
    """The raw raster as the push takes it: (h, w * bpp + pad) uint8, little-endian for gray16; `pad` bytes of `fill` end each row."""
    name = name_of(fmt)
    raw = np.ascontiguousarray(raw)
    h, w = raw.shape[:2]
    if name == "gray16":
        raw = raw.astype("<u2")
    body = raw.view(np.uint8).reshape(h, w * BPP[name])
    if not pad:
        return np.ascontiguousarray(body)
    out = np.full((h, w * BPP[name] + pad), fill, np.uint8)
    out[:, :w * BPP[name]] = body
    return out


KINDS = ["random", "saturated", "stripes_x", "stripes_y", "checker", "ramp", "scene", "lowbits"]


def raw_images(w, h, fmt, seed=0, shift=0):
    """Eight seeded raw images in the format: noise, saturated blocks, the period-2 patterns (the worst case of the Bayer means),
    a ramp, a smooth scene, and values whose low bits the conversion must drop."""
    name = name_of(fmt)
    rng = np.random.default_rng(0x51F7 + 1009 * seed + 31 * FORMATS[name] + 7 * w + h)
    ch = BPP[name] if name in ("rgb8", "bgr8", "rgba8", "bgra8") else 1
    top = 65535 if name == "gray16" else 255
    yy, xx = np.mgrid[0:h, 0:w]

    def chans(f):
        """One plane per channel from f(channel index), stacked for the colour formats."""
        planes = [np.clip(f(c), 0, top).astype(np.int64) for c in range(ch)]
        a = planes[0] if ch == 1 else np.stack(planes, axis=-1)
        return a.astype(np.uint16 if name == "gray16" else np.uint8)

    lo, hi = rng.integers(0, top // 3, 4), rng.integers(2 * top // 3, top + 1, 4)
    out = {
        "random": chans(lambda c: rng.integers(0, top + 1, (h, w))),
        "saturated": chans(lambda c: np.where(((xx // 5 + yy // 3 + c) % 3) == 0, top, np.where(((xx // 5 + yy // 3 + c) % 3) == 1, 0, rng.integers(0, top + 1, (h, w))))),
        "stripes_x": chans(lambda c: np.where((xx + c) & 1, hi[c], lo[c])),
        "stripes_y": chans(lambda c: np.where((yy + c) & 1, hi[c], lo[c]) + (xx & 1)),
        "checker": chans(lambda c: np.where((xx + yy + c) & 1, hi[c], lo[c])),
        "ramp": chans(lambda c: ((xx * (c + 2) + yy * 3) * (top // 255)) % (top + 1)),
        "scene": chans(lambda c: (top / 2) * (1 + np.sin(xx / (5.0 + c)) * np.cos(yy / (7.0 - c))) + rng.integers(0, 3, (h, w))),
        "lowbits": chans(lambda c: (rng.integers(0, 256, (h, w)) << shift) | rng.integers(0, 1 << shift, (h, w)) if name == "gray16"
                         else rng.integers(0, 256, (h, w)) // (c + 1)),
    }
    assert list(out) == KINDS
    return out
