"""The jobs the descriptor matcher is driven with, on the CPU (tests/test_match_reference.py: the header and a double loop
against the numpy restatement) and on the device (tests/test_gpu_match.py).  Seeded and small.  Most train descriptors are a
query descriptor with k bits flipped, so that distances are small and known and not clustered at 128.

CASES is a list of dicts: name, query, train (uint8[n, 32]), query_valid, train_valid (uint8[n] or None), max_distance, ratio,
cross_check, and for the hand-made ones `want`: the idx / nearest / dist / second they must give."""
import numpy as np

import match_reference as MR

T = MR.TILE
NQ = [0, 1, 63, 64, 65, 129]
NT = [0, 1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1]
NONE = MR.NONE


def rand_desc(rng, n):
    return rng.integers(0, 256, (n, 32), dtype=np.uint8)


def flip(desc, bits):
    """A copy of one descriptor with the listed bits flipped."""
    d = np.array(desc, np.uint8).copy()
    for b in bits:
        d[b >> 3] ^= np.uint8(1 << (b & 7))
    return d


def flipped(rng, desc, k):
    return flip(desc, rng.choice(256, k, replace=False))


def near_set(rng, base, n, k_max=12):
    """n descriptors, each one of `base` with 0 .. k_max bits flipped."""
    out = np.zeros((n, 32), np.uint8)
    for j in range(n):
        out[j] = flipped(rng, base[rng.integers(len(base))], int(rng.integers(0, k_max + 1)))
    return out


def edge_validity(n, seed):
    """Invalid at 0, 63, 64 and last (where the set has them), and at a tenth of the rest."""
    rng = np.random.default_rng([n, seed])
    v = (rng.random(n) >= 0.1).astype(np.uint8)
    for k in (0, 63, 64, n - 1):
        if 0 <= k < n:
            v[k] = 0
    return v


def case(name, query, train, query_valid=None, train_valid=None, max_distance=256, ratio=0.0, cross_check=False, want=None):
    q = np.ascontiguousarray(query, dtype=np.uint8).reshape(-1, 32)
    t = np.ascontiguousarray(train, dtype=np.uint8).reshape(-1, 32)
    c = dict(name=name, query=q, train=t, query_valid=None if query_valid is None else np.ascontiguousarray(query_valid, dtype=np.uint8),
             train_valid=None if train_valid is None else np.ascontiguousarray(train_valid, dtype=np.uint8),
             max_distance=max_distance, ratio=ratio, cross_check=bool(cross_check), want=want)
    for k in ("query", "train", "query_valid", "train_valid"):
        if c[k] is not None:
            c[k].setflags(write=False)
    return c


def options(c):
    """What match_reference.match and Context.match take."""
    return {k: c[k] for k in ("query", "train", "query_valid", "train_valid", "max_distance", "ratio", "cross_check")}


def _size_cases():
    out, k = [], 0
    for nq in NQ:
        for nt in NT:
            rng = np.random.default_rng([nq, nt, 11])
            q = rand_desc(rng, nq)
            t = near_set(rng, q if nq else rand_desc(rng, 1), nt)
            kind = k % 4               # 0: plain; 1: train validity; 2: both; 3: query validity
            out.append(case("size %dx%d" % (nq, nt), q, t,
                            query_valid=edge_validity(nq, 1) if kind in (2, 3) else None,
                            train_valid=edge_validity(nt, 2) if kind in (1, 2) else None,
                            max_distance=[256, 9, 4][k % 3], ratio=[0.0, 0.8, 1.0, 0.5][(k // 3) % 4], cross_check=(k // 2) % 2 == 1))
            k += 1
    return out


def _large_cases():
    rng = np.random.default_rng(65535)
    q = rand_desc(rng, 3)
    t = rand_desc(rng, 65535)                       # far from everything: distances around 128
    t[65534] = flip(q[0], [3, 200])                 # the winner is the last index a set can have
    t[1000] = t[65533] = flip(q[1], [7])            # a duplicate: the lower index wins, second == dist
    t[65534 - 64] = q[2]
    big_t = case("3x65535", q, t, ratio=0.8, cross_check=True,
                 want=dict(idx=[65534, -1, 65534 - 64], nearest=[65534, 1000, 65534 - 64], dist=[2, 1, 0]))
    t2 = rand_desc(rng, 2)
    q2 = near_set(rng, t2, 65535, k_max=40)
    v = np.ones(65535, np.uint8)
    v[[0, 63, 64, 65534]] = 0
    return [big_t, case("65535x2", q2, t2, query_valid=v, max_distance=30, cross_check=True)]


def _hand_cases():
    rng = np.random.default_rng(2024)
    a, b, c = rand_desc(rng, 3)
    out = []
    # duplicates: the lowest index wins, and dist == second
    out.append(case("duplicate train", [a, b], [flip(c, [1]), flip(a, [5, 6]), flip(a, [5, 6]), flip(a, [5, 6]), b, b],
                    want=dict(idx=[1, 4], nearest=[1, 4], dist=[2, 0], second=[2, 0])))
    out.append(case("all equal", [a] * 5, [a] * 7, want=dict(idx=[0] * 5, nearest=[0] * 5, dist=[0] * 5, second=[0] * 5)))
    out.append(case("all equal, cross-checked", [a] * 5, [a] * 7, cross_check=True, want=dict(idx=[0, -1, -1, -1, -1], nearest=[0] * 5)))
    out.append(case("distance 0 and 256", [a], [~a, a], want=dict(idx=[1], nearest=[1], dist=[0], second=[256])))
    out.append(case("the complement alone", [a], [~a], want=dict(idx=[0], dist=[256], second=[NONE])))
    out.append(case("the complement alone, max 255", [a], [~a], max_distance=255, want=dict(idx=[-1], nearest=[0], dist=[256], second=[NONE])))
    # validity
    q70, t70 = rand_desc(rng, 70), None
    t70 = near_set(rng, q70, 70, k_max=6)
    out.append(case("edges invalid on both sides", q70, t70, query_valid=edge_validity(70, 3), train_valid=edge_validity(70, 4), cross_check=True))
    out.append(case("all train invalid", q70[:5], t70[:9], train_valid=np.zeros(9, np.uint8),
                    want=dict(idx=[-1] * 5, nearest=[-1] * 5, dist=[NONE] * 5, second=[NONE] * 5)))
    out.append(case("all query invalid", q70[:5], t70[:9], query_valid=np.zeros(5, np.uint8), cross_check=True,
                    want=dict(idx=[-1] * 5, nearest=[-1] * 5, dist=[NONE] * 5, second=[NONE] * 5)))
    one = np.zeros(9, np.uint8)
    one[6] = 1
    out.append(case("exactly one valid train", q70[:5], t70[:9], train_valid=one, ratio=0.5, want=dict(idx=[6] * 5, nearest=[6] * 5, second=[NONE] * 5)))
    # max_distance at dist, at dist - 1, at 0 and at 256
    t5 = [flip(a, [0, 50, 100, 150, 255]), flip(a, range(40))]
    for md, idx in [(5, 0), (4, -1), (0, -1), (256, 0)]:
        out.append(case("max_distance %d, dist 5" % md, [a], t5, max_distance=md, want=dict(idx=[idx], nearest=[0], dist=[5], second=[40])))
    out.append(case("max_distance 0, dist 0", [a], [b, a], max_distance=0, want=dict(idx=[1], dist=[0])))
    # the ratio test: (float)dist < ratio * (float)second in float32
    def pair(d1, d2):
        return [flip(a, range(10, 10 + d2)), flip(a, range(100, 100 + d1))]          # the nearer one second
    out.append(case("ratio off, tie", [a], pair(3, 3), ratio=0.0, want=dict(idx=[0], dist=[3], second=[3])))
    out.append(case("ratio 1.0, tie", [a], pair(3, 3), ratio=1.0, want=dict(idx=[-1], nearest=[0], dist=[3], second=[3])))
    out.append(case("ratio 0.75, 3 against 4", [a], pair(3, 4), ratio=0.75, want=dict(idx=[-1], nearest=[1], dist=[3], second=[4])))       # 3 < 3.0 is false
    out.append(case("ratio 0.8f, 4 against 5", [a], pair(4, 5), ratio=0.8, want=dict(idx=[-1], nearest=[1], dist=[4], second=[5])))        # 0.8f * 5 rounds to 4.0
    out.append(case("ratio 0.8f, 3 against 5", [a], pair(3, 5), ratio=0.8, want=dict(idx=[1], nearest=[1], dist=[3], second=[5])))
    out.append(case("ratio 0.75, 2 against 4", [a], pair(2, 4), ratio=0.75, want=dict(idx=[1], dist=[2], second=[4])))
    lone = np.array([0, 1], np.uint8)
    for r, d1 in [(1.0, 3), (0.75, 3), (0.8, 4)]:
        out.append(case("ratio %g, no second" % r, [a], pair(d1, d1 + 1), train_valid=lone, ratio=r, want=dict(idx=[1], dist=[d1], second=[NONE])))
    # cross-check: bwd(fwd(0)) != 0 ...
    t0 = flip(a, [1, 2, 3, 4])
    out.append(case("cross-check rejects", [a, flip(t0, [9])], [t0], cross_check=True, want=dict(idx=[-1, 0], nearest=[0, 0], dist=[4, 1])))
    out.append(case("cross-check off", [a, flip(t0, [9])], [t0], cross_check=False, want=dict(idx=[0, 0], nearest=[0, 0], dist=[4, 1])))
    # ... and two queries that share their nearest train at one distance: the lower query index has it
    out.append(case("cross-check tie", [b, a, a], [flip(a, [8, 9])], cross_check=True, want=dict(idx=[-1, 0, -1], nearest=[0, 0, 0], second=[NONE] * 3)))
    out.append(case("cross-check tie, the first invalid", [a, a, a], [flip(a, [8, 9])], query_valid=[0, 1, 1], cross_check=True, want=dict(idx=[-1, 0, -1], nearest=[-1, 0, 0])))
    return out


CASES = _hand_cases() + _size_cases() + _large_cases()
assert len({c["name"] for c in CASES}) == len(CASES)
