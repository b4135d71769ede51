"""numpy restatement of the descriptor contract ("Descriptors"), written from the contract and not from
csrc/hip/fe_brief.h: the generated sampling pattern, the validity and centre rule, the 5 x 5 box sums over a replicated border
and the 256 strict comparisons, 32 bytes per point.

MUTATIONS names deliberate mistakes; describe(..., mutation=name) computes what an implementation with that mistake would give
(tests/test_brief_reference.py shows that each changes some expected output)."""
import numpy as np

TESTS, BYTES, REACH, BOX = 256, 32, 12, 2
_M = (1 << 64) - 1

MUTATIONS = ("le_for_lt", "box_radius_1", "swap_ax_ay", "zero_padding", "truncate_without_half", "bit_order_reversed", "swap_t_t64")


def splitmix64(k):
    z = (0xB21EFB21EFB21EF5 + 0x9E3779B97F4A7C15 * k) & _M
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & _M
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & _M
    z ^= z >> 31
    return z


def coordinate(z):
    return z % 9 + (z >> 16) % 9 + (z >> 32) % 9 - 12


def generate_pattern():
    """(tests (256, 4) int64 of ax, ay, bx, by; number of draws)."""
    tests, k = [], 0
    while len(tests) < TESTS:
        ax, ay, bx, by = (coordinate(splitmix64(k + i)) for i in (1, 2, 3, 4))
        k += 4
        if (ax, ay) == (bx, by):
            continue
        tests.append((ax, ay, bx, by))
    return np.array(tests, np.int64), k


PATTERN, DRAWS = generate_pattern()


def valid_and_centre(pts, w, h, mutation=None):
    """(valid bool[n], cx int64[n], cy int64[n]); the centre of an invalid point is 0."""
    pts = np.asarray(pts, np.float32).reshape(-1, 2)
    with np.errstate(invalid="ignore", over="ignore"):
        f = pts + np.float32(0.5)
        assert f.dtype == np.float32
        valid = (f[:, 0] >= 0) & (f[:, 0] < np.float32(w)) & (f[:, 1] >= 0) & (f[:, 1] < np.float32(h))
        src = pts if mutation == "truncate_without_half" else f
        c = np.where(valid[:, None], src, np.float32(0)).astype(np.int64)      # (truncation; the values are in 0 .. w - 1)
    return valid, c[:, 0], c[:, 1]


def box_sums(img, mutation=None):
    """S over the image grown by REACH on every side: out[y + REACH, x + REACH] = S(x, y), int64."""
    img = np.asarray(img)
    assert img.ndim == 2 and img.dtype == np.uint8
    r = 1 if mutation == "box_radius_1" else BOX
    pad = REACH + r
    big = np.pad(img.astype(np.int64), pad, mode="constant" if mutation == "zero_padding" else "edge")
    hh, ww = img.shape[0] + 2 * REACH, img.shape[1] + 2 * REACH
    out = np.zeros((hh, ww), np.int64)
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            out += big[dy:dy + hh, dx:dx + ww]
    return out


def describe(img, pts, mutation=None, sums=None):
    """(desc uint8[n, 32], valid uint8[n]) of the points (x, y in level-0 pixels) of a (h, w) uint8 image."""
    img = np.asarray(img)
    h, w = img.shape
    pts = np.asarray(pts, np.float32).reshape(-1, 2)
    valid, cx, cy = valid_and_centre(pts, w, h, mutation)
    S = box_sums(img, mutation) if sums is None else sums
    pat = PATTERN.copy()
    if mutation == "swap_ax_ay":
        pat = pat[:, [1, 0, 2, 3]]
    if mutation == "swap_t_t64":
        pat = np.concatenate([pat[64:128], pat[:64], pat[128:]])
    ax, ay, bx, by = (pat[None, :, i] for i in range(4))
    Y, X = cy[:, None] + REACH, cx[:, None] + REACH
    sa, sb = S[Y + ay, X + ax], S[Y + by, X + bx]
    bits = (sa <= sb) if mutation == "le_for_lt" else (sa < sb)
    bits = bits & valid[:, None]
    desc = np.packbits(bits.reshape(-1, BYTES, 8), axis=2, bitorder="big" if mutation == "bit_order_reversed" else "little").reshape(-1, BYTES)
    return desc.astype(np.uint8), valid.astype(np.uint8)


def hamming(a, b):
    """Hamming distances of descriptor arrays that broadcast against each other: (.., 32) uint8 -> (..) int."""
    return np.unpackbits(np.bitwise_xor(a, b), axis=-1).sum(axis=-1)
