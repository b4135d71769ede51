"""The descriptor matcher's contract ("Descriptor matching") restated in numpy, written from that list and
not from csrc/hip/fe_match.h: the CPU tests compare the header with it, the GPU tests the kernel and the C ABI.

    distance   d(i, j) = popcount of the XOR of the 32 bytes
    forward    nearest(i) = the valid train of the smallest (d(i, j), j); dist; second = the smallest d(i, j) over valid
               j != nearest(i); -1 / 0xFFFF / 0xFFFF without a valid train or for an invalid query
    backward   bwd(j) = the valid query of the smallest (d(i, j), i)
    accept     nearest >= 0, dist <= max_distance, ratio == 0 or second == 0xFFFF or float32(dist) < float32(ratio) * float32(second),
               and with cross_check bwd(nearest) == i
"""
import numpy as np

BYTES = 32
MAX_N = 65535
NONE = 0xFFFF
TILE = 256                     # FM_TILE: the descriptors the kernel stages at a time (the size cases stand around it)
MATCH = np.dtype([("idx", "<i4"), ("nearest", "<i4"), ("dist", "<u2"), ("second", "<u2")])

_POP8 = np.array([bin(v).count("1") for v in range(256)], np.uint8)
_FAR = 1 << 20                 # more than any distance


def _set(desc, valid):
    d = np.ascontiguousarray(desc, dtype=np.uint8).reshape(-1, BYTES)
    v = np.ones(len(d), bool) if valid is None else np.asarray(valid).reshape(-1) != 0
    assert len(v) == len(d) <= MAX_N
    return d, v


def distances(query, train):
    """(nq, nt) int32 Hamming distances."""
    q = np.ascontiguousarray(query, dtype=np.uint8).reshape(-1, BYTES)
    t = np.ascontiguousarray(train, dtype=np.uint8).reshape(-1, BYTES)
    out = np.zeros((len(q), len(t)), np.int32)
    step = max(1, (1 << 22) // max(1, len(t) * BYTES))             # rows at a time: some MiB of XOR bytes
    for i0 in range(0, len(q), step):
        out[i0:i0 + step] = _POP8[q[i0:i0 + step, None, :] ^ t[None, :, :]].sum(axis=2, dtype=np.int32)
    return out


def match(query, train, query_valid=None, train_valid=None, max_distance=256, ratio=0.0, cross_check=False):
    """(matches MATCH[nq], n_matches)."""
    q, qv = _set(query, query_valid)
    t, tv = _set(train, train_valid)
    nq, nt = len(q), len(t)
    out = np.zeros(nq, MATCH)
    out["idx"], out["nearest"], out["dist"], out["second"] = -1, -1, NONE, NONE
    if nq == 0 or nt == 0 or not tv.any() or not qv.any():
        return out, 0
    d = distances(q, t)
    fwd = np.where(tv[None, :], d, _FAR)
    nearest = fwd.argmin(axis=1)                                   # the first minimum: the lowest index among equal distances
    rows = np.arange(nq)
    dist = fwd[rows, nearest]
    rest = fwd.copy()
    rest[rows, nearest] = _FAR
    second = rest.min(axis=1)
    second = np.where(second >= _FAR, NONE, second)
    ok = qv.copy()                                                 # (a valid train exists: every valid query has a nearest)
    out["nearest"][ok] = nearest[ok]
    out["dist"][ok] = dist[ok]
    out["second"][ok] = second[ok]
    acc = ok & (dist <= max_distance)
    r = np.float32(ratio)
    if r != 0:
        acc &= (second == NONE) | (dist.astype(np.float32) < r * second.astype(np.float32))
    if cross_check:
        bwd = np.where(qv[:, None], d, _FAR).argmin(axis=0)        # per train: the lowest query index among equal distances
        acc &= bwd[nearest] == rows
    out["idx"][acc] = nearest[acc]
    return out, int(acc.sum())
