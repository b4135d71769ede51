"""The arithmetic contract of the published odometry covariance (tests/odom_cov_reference.py) on the CPU:
the fixed-order form agrees with the reference's literal H P H^T to rounding, and every plausible mistake (block order,
transposed rotation, wrong velocity block, no rotation) is many orders of magnitude beyond that rounding."""
import numpy as np

import odom_cov_reference as OC

N_INPUTS = 200


def _inputs():
    """200 seeded symmetric positive-definite P, d = 21 + 6 k for k = 0..4, per-state scales 1e-4 .. 1e1, each with a rotation
    of its own (0.4 .. 2.6 rad about a random axis: never near the identity, never symmetric)."""
    rng = np.random.default_rng(0x0D0C)
    out = []
    for n in range(N_INPUTS):
        d = 21 + 6 * (n % 5)
        A = rng.normal(size=(d, d))
        S = A @ A.T / d + np.eye(d)
        s = 10.0 ** rng.uniform(-4, 1, size=d)
        P = S * np.outer(s, s)
        P = (P + P.T) / 2
        R = OC.rotation(rng.normal(size=3), rng.uniform(0.4, 2.6))
        out.append((P, R))
    return out


INPUTS = _inputs()


def _distance(a, b, bar):
    """max over the entries of |a - b| in units of the entry's bar"""
    return float((np.abs(np.asarray(a, dtype=OC.LD) - np.asarray(b, dtype=OC.LD)) / bar).max())


def test_fixed_order_agrees_with_the_literal_reference():
    """Entry by entry within 8 eps (|R| |B| |R|^T)_ij: two nested 3-term dot products give gamma_6 ~ 6 eps, the 8 leaves room
    for the long-double side.  Observed: 2.0 eps in those units at worst."""
    worst = 0.0
    for P, R in INPUTS:
        assert np.array_equal(P, P.T) and np.linalg.eigvalsh(P).min() > 0
        pose, twist, pv = OC.odom_cov_fixed(P, R)
        lpose, ltwist, lpv = OC.odom_cov_literal(P, R)
        bpose, btwist = OC.error_bar(P, R)
        e = max(_distance(pose, lpose, bpose), _distance(twist, ltwist, btwist))
        assert e <= 1.0, e
        worst = max(worst, e)
        assert np.array_equal(pv, np.diag(P)[12:15]) and np.array_equal(pv, np.asarray(lpv, dtype=np.float64))
    print("fixed against literal: worst %.2f of the bar = %.2f eps (|R||B||R|^T)" % (worst, 8 * worst))


MUTANTS = {
    "orientation block first": lambda P, R: OC.odom_cov_fixed(P, R, blocks={(0, 0): (0, 0), (0, 3): (0, 12), (3, 0): (12, 0), (3, 3): (12, 12)}),
    "R^T for R": lambda P, R: OC.odom_cov_fixed(P, np.ascontiguousarray(R.T)),
    "velocity from P[3:6, 3:6]": lambda P, R: OC.odom_cov_fixed(P, R, vel=3),
    "no rotation": lambda P, R: OC.odom_cov_fixed(P, R, rotate=False),
}


def test_mutations_are_far_beyond_the_bar():
    """Each wrong variant differs from the contract by at least 1e6 bars on every input (observed: >= 1e13), so the bitwise
    GPU tests and the bar above cannot pass by accident."""
    smallest = {}
    for name, f in MUTANTS.items():
        for P, R in INPUTS:
            pose, twist, _ = OC.odom_cov_fixed(P, R)
            mpose, mtwist, _ = f(P, R)
            bpose, btwist = OC.error_bar(P, R)
            dist = max(_distance(pose, mpose, bpose), _distance(twist, mtwist, btwist))
            assert dist >= 1e6, (name, dist)
            smallest[name] = min(smallest.get(name, np.inf), dist)
    print("smallest distance per mutant, in bars:", {k: "%.1e" % v for k, v in smallest.items()})
