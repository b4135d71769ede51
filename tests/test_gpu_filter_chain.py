"""The measurement update on the plane a run leaves behind: windows that are partly filled (d well below ld) and a dead region
that holds old numbers a million times larger than P (tests/chain_cases.py; tests/test_chain_cases.py is its CPU proof).

Every other update test starts from mskf_ekf_set_cov on a stream whose capacity equals the problem's window, so the launches
sized from max_d and the classes chosen from S.d coincide and everything beyond [0, d) x [0, d) is zero.  Here the same
problems of update_cases.CASES run at capacity window + 6, and those up to 31 clones at capacity 64 too, after the dead
region was poisoned through mskf_ekf_set_cov + four mskf_ekf_remove_clones_batch calls (chain_cases: why four and not three).

Bars: those of tests/update_cases.py, unchanged (Householder and uncompressed routes D_P < 1e-12, D_x < 1e-9; Gram route 1e-9
against update_with_prior and 1e-6 against the plain update); test_gpu_update_routes._check is restated here verbatim.  On top:
bitwise equality with the same update on a full-window stream, and a dead region that is bit-identical before and after.
No route needed an exception from either: no order of summation depends on ld and no kernel writes beyond [0, d) x [0, d).

The second half carries ONE stream of capacity 45 through the whole filter cycle (test_chain_step_by_step).

Measured on an MI355X (DESIGN.md section 1 has the figures per family).  Roomy windows, being bitwise the full-window updates,
repeat test_gpu_update_routes: Householder and uncompressed D_P <= 2.0e-15, D_x <= 9.5e-13; Gram against update_with_prior
D_P <= 2.0e-14, D_x <= 1.7e-13, against the plain update 2.2e-10.  Chain, per call against the step from the device's own P:
prediction <= 6.6e-16 per block; Householder D_P <= 5.0e-16, D_x <= 4.5e-13; uncompressed 8.2e-17, 3.5e-14; Gram (mode 1)
against update_with_prior 2.2e-15, 4.5e-13, against the plain update 1.8e-9.  End-of-chain distance from a long-double chain that
carries its own P: 2.1e-15 after the 99 calls of mode 3; 1.2e-8 after the 64 calls of mode 1 (the Gram route's lambda I, summed).
"""
import numpy as np
import pytest

from msckf_stereo_c_amd import capi
from msckf_stereo_c_amd.ctypes_types import default_ekf_cfg, default_fe_cfg

import chain_cases as CC
import feature_reference as FR
import update_cases as U

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not FR.HAVE_LONG_DOUBLE, reason=FR.NEED_LONG_DOUBLE)]


def _kwargs(c):
    return dict(gravity=c["gravity"].copy(), clones=c["clones"].copy(), positions=c["positions"].copy(), obs_start=c["obs_start"].copy(),
                obs_clone=c["obs_clone"].copy(), obs_z=c["obs_z"].copy(), dof_offset=c["dof_offset"], apply_row_cap=c["apply_row_cap"])


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _full_stream(ctx, c):
    s = capi.Stream(ctx, c["calib"], default_fe_cfg(), default_ekf_cfg(max_cam_state_size=c["window"], compression_mode=c["mode"]))
    s.ekf_set_cov(c["P"])
    return s


_FULL = {}


def _full_window(ctx, c):
    """The update on a stream born with the problem's window (what test_gpu_update_routes runs), once per case."""
    if c["name"] not in _FULL:
        s = _full_stream(ctx, c)
        got = s.ekf_update(**_kwargs(c))
        _FULL[c["name"]] = (got, s.ekf_get_cov())
        s.close()
    return _FULL[c["name"]]


def _roomy_stream(ctx, c, capacity):
    """A stream of `capacity` clones that holds the case's P in a poisoned plane; the three preconditions are asserted here.
    Returns (stream, the whole plane before the update)."""
    s = capi.Stream(ctx, c["calib"], default_fe_cfg(), default_ekf_cfg(max_cam_state_size=capacity, compression_mode=c["mode"]))
    s.ekf_set_cov(CC.poisoned_full(c["P"], U.PROBLEMS[c["problem"]]["seed"]))
    for pair in CC.removals(c["window"]):
        ctx.ekf_remove_clones_batch([s], [pair])
    assert s.ekf_dim() == c["d"]
    assert np.array_equal(_bits(s.ekf_get_cov()), _bits(c["P"]))
    plane = s.ekf_debug_plane()
    assert plane.shape == (CC.ld_of(capacity),) * 2
    assert np.array_equal(_bits(plane[:c["d"], :c["d"]]), _bits(c["P"]))
    assert CC.near_dead_is_poisoned(plane, c["d"], c["P"])
    return s, plane


def _same_bits(a, Pa, b, Pb):
    assert a["rows"] == b["rows"] and a["used_qr"] == b["used_qr"]
    assert np.array_equal(a["status"], b["status"])
    assert np.array_equal(_bits(a["gamma"]), _bits(b["gamma"]))
    assert np.array_equal(_bits(a["delta_x"]), _bits(b["delta_x"]))
    assert np.array_equal(_bits(Pa), _bits(Pb))


def _dead_untouched(c, before, after):
    dead = CC.dead_mask(len(before), c["d"])
    changed = np.argwhere(dead & (_bits(before) != _bits(after)))
    assert len(changed) == 0, "dead entries written by the update, first %s of %d" % (changed[:4].tolist(), len(changed))


def _check(c, got, Pg, tag):
    """test_gpu_update_routes._check, with the figures printed under `tag`."""
    s = U.stack(c["problem"])
    assert got["rows"] == c["st"]
    assert np.array_equal(got["status"] & 1, np.ones(len(c["specs"]), np.uint8))
    assert np.array_equal(((got["status"] >> 1) & 1).astype(bool), s["passed"])
    assert got["used_qr"] == c["used_qr"]
    assert np.array_equal(_bits(Pg), _bits(Pg.T.copy()))
    plain = U.reference(c["problem"])
    D_P, D_x = U.distances(got["delta_x"], Pg, plain)
    bar = U.GRAM_BAR if c["gram"] else U.HH_P_BAR
    min_eig = float(np.linalg.eigvalsh(Pg).min()) / float(np.abs(c["P"]).max())
    line = "%s %s (%s, mode %d, used_qr %d): plain reference D_P %.3e, D_x %.3e" % (tag, c["name"], c["family"], c["mode"], got["used_qr"], D_P, D_x)
    G_P = G_x = B_P = B_x = 0.0
    if c["gram"]:
        G_P, G_x = U.distances(got["delta_x"], Pg, U.reference_with_prior(c["problem"]))
        line += "; update_with_prior D_P %.3e, D_x %.3e" % (G_P, G_x)
    if c["inflated"] is not None:
        B_P, B_x = U.distances(got["delta_x"], Pg, plain, exclude=c["inflated"])
        line += "; without state %d D_P %.3e, D_x %.3e" % (c["inflated"], B_P, B_x)
    print(line + "; min eig(P') / max|P| %.3e" % min_eig)
    if c["gram"]:
        assert G_P < U.GRAM_BAR and G_x < U.GRAM_BAR
        assert D_P < U.GRAM_PLAIN_BAR
    else:
        assert D_P < U.HH_P_BAR and D_x < U.HH_X_BAR
        assert B_P < U.HH_P_BAR and B_x < U.HH_X_BAR
    assert min_eig >= -bar


@pytest.mark.parametrize("name,capacity", CC.ROOMY_RUNS, ids=["%s-cap%d" % r for r in CC.ROOMY_RUNS])
def test_update_on_a_partly_filled_poisoned_window(gpu_ctx, name, capacity):
    """One case of update_cases.CASES on a stream of `capacity` clones (d = 21 + 6 window, ld = align_up(21 + 6 capacity, 8))
    whose dead rows and columns hold 1e6 max|P|: rows, status, used_qr, the distances at the bars of update_cases, bitwise
    symmetry and min eig(P') as test_gpu_update_routes asserts them; status, gamma, delta_x and the live block of P' bitwise
    those of the same update on a stream of capacity `window`; and not one bit of the dead region changed."""
    c = U.case(name)
    s, before = _roomy_stream(gpu_ctx, c, capacity)
    got = s.ekf_update(**_kwargs(c))
    Pg = s.ekf_get_cov()
    after = s.ekf_debug_plane()
    s.close()
    assert np.array_equal(_bits(after[:c["d"], :c["d"]]), _bits(Pg))
    _check(c, got, Pg, "capacity %d" % capacity)
    full, P_full = _full_window(gpu_ctx, c)
    _same_bits(full, P_full, got, Pg)
    _dead_untouched(c, before, after)


def test_roomy_streams_in_one_batch_are_bitwise_the_updates_alone(gpu_ctx):
    """One mskf_ekf_update_batch over two streams of capacity 64 that hold 30 clones (mode 1, k_ekf_chol_lds) and 43 clones
    (mode 3, k_ekf_tsqr<16,4,2>) in poisoned planes, beside a 5-clone stream that fills its window: the launch is sized for
    ld = 408 while the three classes come from d = 201, 279 and 51.  Each stream is bitwise its update alone on a stream of
    the same capacity, and the dead regions are untouched."""
    cases = [U.case(n) for n in CC.ROOMY_BATCH]
    alone = []
    for c, cap in zip(cases, (CC.WIDE, CC.WIDE, None)):
        if cap is None:
            alone.append(_full_window(gpu_ctx, c))
            continue
        s, _ = _roomy_stream(gpu_ctx, c, cap)
        got = s.ekf_update(**_kwargs(c))
        alone.append((got, s.ekf_get_cov()))
        s.close()
    made = [_roomy_stream(gpu_ctx, cases[0], CC.WIDE), _roomy_stream(gpu_ctx, cases[1], CC.WIDE), (_full_stream(gpu_ctx, cases[2]), None)]
    ss = [m[0] for m in made]
    together = gpu_ctx.ekf_update_batch(ss, [_kwargs(c) for c in cases])
    P_together = [s.ekf_get_cov() for s in ss]
    planes = [s.ekf_debug_plane() for s in ss]
    for s in ss:
        s.close()
    for c, (a, Pa), b, Pb, (_, before), after in zip(cases, alone, together, P_together, made, planes):
        _check(c, b, Pb, "batch")
        _same_bits(a, Pa, b, Pb)
        if before is not None:
            _dead_untouched(c, before, after)


# ---------------------------------------------------------------------------------------------- the carried chain
import ekf_reference as R            # noqa: E402

PREDICT_BAR = 1e-12                  # tests/test_gpu_filter_predict.py, per block
SEGMENT_COST = 5e7                   # sum of st d^2 per test: well under a second of long-double updates, gates and predictions on top


def _segments(mode):
    """The chain's op indices cut where the long-double cost of the updates so far passes SEGMENT_COST."""
    _, ops = CC.chain_ops(mode)
    out, start, cost = [], 0, 0.0
    for i, o in enumerate(ops):
        if o["op"] == "update":
            cost += o["st"] * o["d"] ** 2 * (2 if CC.used_qr(o, mode) == 0 else 1)
        if cost >= SEGMENT_COST:
            out.append((start, i + 1))
            start, cost = i + 1, 0.0
    if start < len(ops):
        out.append((start, len(ops)))
    return out


SEGMENTS = [(m, a, b) for m in (CC.FULL_MODE, CC.GRAM_MODE) for a, b in _segments(m)]
_DEVICE, _CARRIED = {}, {}


def _device_chain(ctx, mode):
    """The whole chain on ONE stream of capacity 45, started with mskf_ekf_reset; mskf_ekf_set_cov is never called.  After every
    call the covariance and the whole plane are read back (reading changes nothing on the device).  Once per mode."""
    if mode in _DEVICE:
        return _DEVICE[mode]
    P0, ops = CC.chain_ops(mode)
    calib = next(o for o in ops if o["op"] == "update")["calib"]
    s = capi.Stream(ctx, calib, default_fe_cfg(), default_ekf_cfg(max_cam_state_size=CC.CAPACITY, compression_mode=mode))
    s.ekf_reset(P0)
    rec = [dict(P=s.ekf_get_cov(), plane=s.ekf_debug_plane(), got=None)]
    for o in ops:
        got = None
        if o["op"] == "predict":
            ctx.ekf_predict_batch([s], [o["steps"]], [o["J"]])
        elif o["op"] == "remove":
            ctx.ekf_remove_clones_batch([s], [o["pair"]])
        else:
            got = s.ekf_update(**_kwargs(o))
        rec.append(dict(P=s.ekf_get_cov(), plane=s.ekf_debug_plane(), got=got, d=s.ekf_dim()))
    s.close()
    _DEVICE[mode] = rec
    return rec


def _carried(mode, upto):
    """The long-double chain that carries its own P (never re-seeded), advanced to just before op `upto`."""
    P0, ops = CC.chain_ops(mode)
    i, P = _CARRIED.get(mode, (0, np.asarray(P0, dtype=CC.LD)))
    if i > upto:
        i, P = 0, np.asarray(P0, dtype=CC.LD)
    qc = R.qc_of(default_ekf_cfg())
    for o in ops[i:upto]:
        if o["op"] == "predict":
            P = CC.ref_predict(P, o, qc)
        elif o["op"] == "remove":
            P = CC.delete_clones(P, o["pair"])
        else:
            P = CC.ref_update(o, P, CC.ref_gates(o, P), False)[0][1]
    _CARRIED[mode] = (upto, P)
    return P


def _outside_untouched(before, after, live, what):
    """Every entry of the plane outside [0, live) x [0, live) has the bits it had."""
    changed = np.argwhere(CC.dead_mask(len(before), live) & (_bits(before) != _bits(after)))
    assert len(changed) == 0, "%s wrote dead entries, first %s of %d" % (what, changed[:4].tolist(), len(changed))


@pytest.mark.parametrize("mode,first,last", SEGMENTS, ids=["mode%d-ops%d-%d" % s for s in SEGMENTS])
def test_chain_step_by_step(gpu_ctx, mode, first, last):
    """Ops [first, last) of chain_cases.build_chain on the one stream that ran the whole chain (capacity 45, mskf_ekf_reset, no
    set_cov; partly filled on every step but one; after the first pruning on the swapped plane, after the second on the first
    plane again, whose dead region then holds the 45-clone covariance of two removals before).  Every step is judged against
    the long-double step computed from the DEVICE's own previous P, at the per-call bars the project already has:
      prediction  per block 1e-12 (test_gpu_filter_predict), P_CC bit for bit;
      update      the bars of update_cases (mode 1: against update_with_prior), rows, status, used_qr as U.predicted gives them,
                  every gate decision the reference's;
      removal     numpy deletion, bit for bit;
    with exact symmetry, min eig(P') >= -bar max|P|, and a dead region that no call touches outside the rows and columns it makes
    live (a removal's new plane holds, outside the block it writes, what that plane held when it was last current).  The
    last segment prints the distance of the device from a long-double chain that carries its own P (a figure, no assertion)."""
    P0, ops = CC.chain_ops(mode)
    rec = _device_chain(gpu_ctx, mode)
    qc = R.qc_of(default_ekf_cfg())
    worst = {}
    # the plane that is not current, as it was when last read: all zero until the first removal (the pool is zero-filled)
    idle = np.zeros_like(rec[0]["plane"])
    for i, o in enumerate(ops[:first]):
        if o["op"] == "remove":
            idle = rec[i]["plane"]
    for i in range(first, last):
        o, before, after = ops[i], rec[i], rec[i + 1]
        Pb, Pa = before["P"], after["P"]
        d = len(Pb)
        assert np.array_equal(_bits(Pa), _bits(Pa.T.copy())), i
        assert np.array_equal(_bits(after["plane"][:after["d"], :after["d"]]), _bits(Pa)), i
        if o["op"] == "predict":
            assert after["d"] == d + 6
            assert np.array_equal(_bits(Pa[CC.N:d, CC.N:d]), _bits(Pb[CC.N:, CC.N:])), i
            err = CC.predict_errors(Pa, CC.ref_predict(Pb, o, qc), d)
            for k, e in err.items():
                worst[("predict", k)] = max(worst.get(("predict", k), 0.0), e)
                assert e <= PREDICT_BAR, (i, k, e)
            _outside_untouched(before["plane"], after["plane"], d + 6, "op %d (prediction)" % i)
        elif o["op"] == "remove":
            assert after["d"] == d - 12
            assert np.array_equal(_bits(Pa), _bits(CC.delete_clones(Pb, o["pair"]))), i
            _outside_untouched(idle, after["plane"], d - 12, "op %d (removal)" % i)
            idle = before["plane"]
        else:
            got = after["got"]
            assert after["d"] == d == o["d"]
            gram = CC.used_qr(o, mode) == 0
            g = CC.ref_gates(o, Pb)
            assert got["rows"] == o["st"] and got["used_qr"] == CC.used_qr(o, mode), (i, got["rows"], got["used_qr"])
            assert np.array_equal(got["status"] & 1, np.ones(len(o["specs"]), np.uint8)), i
            assert np.array_equal(((got["status"] >> 1) & 1).astype(bool), g["passed"]) and g["passed"].all(), i
            plain, prior = CC.ref_update(o, Pb, g, gram)
            D_P, D_x = U.distances(got["delta_x"], Pa, plain)
            key = "gram" if gram else {1: "householder", 2: "uncompressed"}[got["used_qr"]] + (" pairs" if o["kind"] == "pairs" else " small" if o["route"] == "small" else "")
            if gram:
                G_P, G_x = U.distances(got["delta_x"], Pa, prior)
                worst[(key, "G_P")], worst[(key, "G_x")] = max(worst.get((key, "G_P"), 0.0), G_P), max(worst.get((key, "G_x"), 0.0), G_x)
                assert G_P < U.GRAM_BAR and G_x < U.GRAM_BAR and D_P < U.GRAM_PLAIN_BAR, (i, o["n"], G_P, G_x, D_P)
            else:
                assert D_P < U.HH_P_BAR and D_x < U.HH_X_BAR, (i, o["n"], o["kind"], D_P, D_x)
            worst[(key, "D_P")], worst[(key, "D_x")] = max(worst.get((key, "D_P"), 0.0), D_P), max(worst.get((key, "D_x"), 0.0), D_x)
            min_eig = float(np.linalg.eigvalsh(Pa).min()) / float(np.abs(Pb).max())
            assert min_eig >= -(U.GRAM_BAR if gram else U.HH_P_BAR), (i, min_eig)
            _outside_untouched(before["plane"], after["plane"], d, "op %d (update, %s at %d clones)" % (i, o["kind"], o["n"]))
    print("mode %d ops %d..%d: %s" % (mode, first, last - 1, ", ".join("%s %s %.2e" % (k[0], k[1], v) for k, v in sorted(worst.items()))))
    P_own = _carried(mode, last)
    if last == len(ops):
        print("mode %d: end of chain (%d calls), device against the long-double chain that carries its own P: max|dP| / max|P| = %.3e" % (
            mode, len(ops), CC.rel(rec[-1]["P"], P_own)))
