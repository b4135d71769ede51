"""The images, sizes and points the descriptor is driven with, on the CPU (tests/test_brief_reference.py: the header against
the numpy restatement) and on the device (tests/test_gpu_describe.py: the kernel against the restatement).

Sizes: one pixel, smaller than the 29 x 29 footprint in both directions, exactly the footprint, one and two more, the
smallest size a stream accepts, an odd size whose rows lie further apart than its width, and a larger odd one.  Image kinds:
those of tests/lk_cases.py and tests/detector_cases.py.  Points: a sub-pixel lattice, every centre of the four 15 x 15 corner
blocks, every distance 0 .. 14 from each side at three places along it, and the validity rule's edge values on both axes."""
import numpy as np

import brief_reference as BR
import detector_cases as DC
import lk_cases as LK

SIZES = [(1, 1), (5, 3), (29, 29), (30, 31), (64, 64), (129, 71), (333, 251)]          # w, h
PITCH = {(129, 71): 141}                                                               # bytes between rows where not w
KINDS = ["smooth", "blocks", "edges", "checker1", "random"]
FOOT = BR.REACH + BR.BOX                                                               # 14

_images = {}


def image(kind, w, h, seed=7):
    key = (kind, w, h, seed)
    if key not in _images:
        if kind == "smooth":
            img = LK.crop(LK.smooth_canvas(w, h, seed), w, h)
        elif kind == "blocks":
            img = LK.crop(LK.block_canvas(w, h, 4, seed), w, h)
        elif kind == "edges":
            img = LK.crop(LK.edge_canvas(w, h, seed), w, h)
        else:
            img = DC.image(kind, w, h, seed)
        img = np.ascontiguousarray(img, dtype=np.uint8)
        assert img.shape == (h, w)
        img.setflags(write=False)
        _images[key] = img
    return _images[key]


def padded(img, pitch):
    """The image in rows `pitch` bytes apart, the bytes between the rows of another value than any neighbour's."""
    h, w = img.shape
    buf = np.full((h, pitch), 0xA5, np.uint8)
    buf[:, :w] = img
    return buf


def lattice(w, h, pitch=7, offset=0.37):
    xs, ys = np.arange(offset, w, pitch), np.arange(offset, h, pitch)
    return np.array([(x, y) for y in ys for x in xs], np.float32).reshape(-1, 2)


def border_centres(w, h):
    """Integer points: all of an image up to 2 FOOT + 2 wide or high in that direction, else the bands described above."""
    def axis(n):
        if n <= 2 * FOOT + 2:
            return list(range(n)), list(range(n))
        edge = list(range(FOOT + 1)) + list(range(n - FOOT - 1, n))
        return edge, sorted({int(n * 0.31), n // 2, int(n * 0.68)})
    ex, mx = axis(w)
    ey, my = axis(h)
    pts = {(x, y) for x in ex for y in ey} | {(x, y) for x in ex for y in my} | {(x, y) for x in mx for y in ey}
    return np.array(sorted(pts), np.float32).reshape(-1, 2)


def validity_edges(w, h):
    """The edge values of the validity rule on one axis, the other in the middle of the image, and the other way round."""
    def values(n):
        f = np.float32
        v = [-0.5, -0.50000006, n - 0.5, n - 0.50000006, np.nextafter(f(n - 0.5), f(-np.inf)), np.nextafter(f(-0.5), f(0)),
             0.49999997, 0.5, n - 1 + 0.49999997, n // 2 + 0.49999997, n // 2 + 0.5, -1.0, float(n), np.nan, np.inf, -np.inf, 1e30, -1e30]
        return [float(f(x)) for x in v]
    mid_x, mid_y = np.float32(w // 2), np.float32(h // 2)
    pts = [(x, mid_y) for x in values(w)] + [(mid_x, y) for y in values(h)] + [(np.nan, np.nan), (np.inf, -0.5), (-0.5, -0.5)]
    return np.array(pts, np.float32).reshape(-1, 2)


def points(w, h):
    return np.concatenate([lattice(w, h), border_centres(w, h), validity_edges(w, h)])


# point counts of the direct launches: none, one, a wavefront's worth of points less one, exactly, one more, and several hundred
COUNTS = [0, 1, 63, 64, 65, 257]


def counted_points(w, h, n, seed=0):
    """n points: the validity edges and border centres first (as many as fit), the rest at random inside and just outside."""
    rng = np.random.default_rng([w, h, n, seed])
    fixed = np.concatenate([validity_edges(w, h), border_centres(w, h)])
    rng.shuffle(fixed)
    rnd = np.stack([rng.uniform(-2, w + 2, n), rng.uniform(-2, h + 2, n)], axis=1).astype(np.float32)
    k = min(len(fixed), n // 2)
    return np.ascontiguousarray(np.concatenate([fixed[:k], rnd[:n - k]]), dtype=np.float32).reshape(-1, 2)
