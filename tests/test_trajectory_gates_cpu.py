"""frx_trajectory_gates without a device: the host-only entries (frx_gate_from_corners, frx_gate_flags), the argument errors of all four entries, and the
restatement (tests/gates_reference.py) against closed forms, planted errors and an independent long-double sampler.  The device kernel is held to the
restatement bit for bit in tests/test_gpu_trajectory_gates.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import extrema_states as es  # noqa: E402
import gate_states as gs  # noqa: E402
import gates_reference as gr  # noqa: E402

INVALID_ARG, NO_DEVICE = -1, -2
GATE_SEED = 5                                                            # seed of the random gates of test_restatement_against_the_long_double_sampler


def _params(sc):
    p = sc.ZHANGJIAJIE
    return (p["horiz_half_len"], p["horiz_half_len"], p["vert_half_len"]), p["grav_acc"]


def _corners(c, a, b):
    c, a, b = (np.asarray(x, dtype=np.float64) for x in (c, a, b))
    return np.array([c - a - b, c + a - b, c + a + b, c - a + b])


def test_gate_from_corners_exact_rectangles(frx):
    """corners that are binary fractions: centre and half edges come back exactly, the fit is exactly (0, 0); fit may be left out"""
    recs = [((0.0, 2.0, 1.0), (1.0, 0.0, 0.0), (0.0, 0.0, -0.5)), ((4.0, -2.0, 1.5), (0.0, 0.75, 0.0), (0.25, 0.0, 0.0)),
            ((-1.0, 0.5, 2.0), (0.5, 0.5, 0.0), (0.0, 0.0, 1.25))]
    corners = np.array([_corners(*r) for r in recs])
    gates, fit = frx.gate_from_corners(corners, with_fit=True)
    assert np.array_equal(gates, np.array([np.concatenate(r) for r in recs]))
    assert np.array_equal(fit, np.zeros((3, 2)))
    assert np.array_equal(frx.gate_from_corners(corners), gates)
    assert np.array_equal(frx.gate_from_corners(corners[1]), gates[1:2])


def test_gate_from_corners_rotated_and_skewed(frx):
    """a rotated rectangle against numpy to 1e-15; a skewed quadrilateral reports how far from a rectangle it is"""
    rng = np.random.default_rng(2)
    Q, _ = np.linalg.qr(rng.normal(0.0, 1.0, (3, 3)))
    c, a, b = np.array([0.75, -0.5, 0.375]), 0.8 * Q[:, 0], 0.45 * Q[:, 1]
    cr = _corners(c, a, b)
    gates, fit = frx.gate_from_corners(cr[None], with_fit=True)
    want = np.concatenate([cr.mean(axis=0), ((cr[1] - cr[0]) + (cr[2] - cr[3])) / 4, ((cr[3] - cr[0]) + (cr[2] - cr[1])) / 4])
    assert np.abs(gates[0] - want).max() <= 1e-15 and np.abs(gates[0] - np.concatenate([c, a, b])).max() <= 1e-15
    assert abs(fit[0, 0]) <= 1e-15 and fit[0, 1] <= 1e-15
    # a parallelogram: a = (1, 0, 0), b = (0.5, 0, 1) - the corners ARE c -/+ a -/+ b, the edges are not orthogonal
    sk = _corners((0.0, 0.0, 1.0), (1.0, 0.0, 0.0), (0.5, 0.0, 1.0))
    g2, f2 = frx.gate_from_corners(sk[None], with_fit=True)
    assert np.array_equal(g2[0], [0.0, 0.0, 1.0, 1.0, 0.0, 0.0, 0.5, 0.0, 1.0])
    assert abs(f2[0, 0] - 0.5 / np.sqrt(1.25)) <= 1e-15 and f2[0, 1] == 0.0
    # one corner of the unit square pulled out of the plane by 1: every corner is 1 / 4 off the best record, in alternating directions
    tw = _corners((0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (0.0, 0.0, 1.0))
    tw[2, 1] += 1.0
    g3, f3 = frx.gate_from_corners(tw[None], with_fit=True)
    assert np.array_equal(g3[0], [0.0, 0.25, 0.0, 1.0, 0.25, 0.0, 0.0, 0.25, 1.0])
    assert abs(f3[0, 0] - 0.0625 / 1.0625) <= 1e-15 and f3[0, 1] == 0.25


def _row(n_pass, time, n_cross=None, nan=False):
    r = np.array([n_pass if n_cross is None else n_cross, n_pass, 0.25 if n_pass else -0.5, time, 0.0, 0.1, 0.1, 0.5, 0.15, 2.0])
    if nan:
        r[:] = np.nan
    return r


def test_gate_flags_against_the_restatement(frx):
    """made-up rows: every flag alone, together, none; candidates without gates; the no-crossing row's -inf is no NONFINITE"""
    none = np.array([0.0, 0.0, -np.inf, 0.0, -1.0, 0.0, 0.0, 0.0, 0.0, 0.0])
    cands = [([_row(1, 1.0), _row(1, 2.0)], 0), ([_row(0, 1.0, n_cross=2)], gr.FLAG_MISSED), ([none], gr.FLAG_MISSED), ([_row(2, 1.0)], gr.FLAG_REPEAT),
             ([_row(1, 2.0), _row(1, 1.0)], gr.FLAG_ORDER), ([_row(1, 1.0), _row(1, 1.0)], gr.FLAG_ORDER), ([_row(1, 1.0, nan=True)], gr.FLAG_NONFINITE),
             ([], 0), ([_row(1, 3.0), _row(0, 0.5), _row(1, 4.0)], gr.FLAG_MISSED),          # a missed gate's TIME plays no part in the order
             ([_row(3, 2.0), none, _row(1, 1.5), _row(1, 9.0, nan=True)], 15), ([], 0)]
    rows = np.array([r for c, _ in cands for r in c])
    off = np.concatenate([[0], np.cumsum([len(c) for c, _ in cands])]).astype(np.int32)
    want = np.array([f for _, f in cands], np.uint32)
    assert np.array_equal(gr.flags_of(rows, off), want)
    assert np.array_equal(frx.gate_flags(rows, off), want)
    assert (frx.GATE_FLAG_MISSED, frx.GATE_FLAG_REPEAT, frx.GATE_FLAG_ORDER, frx.GATE_FLAG_NONFINITE) == (1, 2, 4, 8)
    assert frx.GATE_FIELDS == gr.FIELDS


def test_argument_errors_come_before_the_device(frx):
    L = frx.lib()
    for name in ("frx_gate_from_corners", "frx_trajectory_gates", "frx_trajectory_gates_device", "frx_gate_flags"):
        assert name in frx.ABI_SYMBOLS and hasattr(L, name)
    buf = np.zeros(64)
    off = np.array([0, 1], np.int32)
    d, o = buf.ctypes.data, off.ctypes.data
    assert L.frx_gate_from_corners(0, d, d, None) == INVALID_ARG
    assert L.frx_gate_from_corners(-1, d, d, d) == INVALID_ARG
    assert L.frx_gate_from_corners(1, None, d, None) == INVALID_ARG
    assert L.frx_gate_from_corners(1, d, None, None) == INVALID_ARG
    assert L.frx_gate_from_corners(1, d, d + 256, None) == 0             # fit may be NULL
    assert L.frx_gate_flags(0, o, d, d) == INVALID_ARG
    assert L.frx_gate_flags(1, None, d, d) == INVALID_ARG
    assert L.frx_gate_flags(1, o, None, d) == INVALID_ARG
    assert L.frx_gate_flags(1, o, d, None) == INVALID_ARG
    assert L.frx_gate_flags(1, np.array([1, 1], np.int32).ctypes.data, d, d) == INVALID_ARG
    assert L.frx_gate_flags(2, np.array([0, 2, 1], np.int32).ctypes.data, d, d) == INVALID_ARG
    h = 8                                                                # never read: these checks come first
    for k in range(6):
        args = [h, 8, 8, 8, 8, 8, 8]
        args[k] = None
        assert L.frx_trajectory_gates(*args) == INVALID_ARG, k
    for k in (0, 1, 2, 4, 5, 6):
        args = [h, 8, 8, 1, 8, 8, 8, None]
        args[k] = None
        assert L.frx_trajectory_gates_device(*args) == INVALID_ARG, k
    assert L.frx_trajectory_gates_device(h, 8, 8, 0, 8, 8, 8, None) == INVALID_ARG
    if L.frx_device_count() < 1:
        assert L.frx_trajectory_gates(h, 8, 8, 8, 8, 8, None) == NO_DEVICE
        assert L.frx_trajectory_gates_device(h, 8, 8, 1, 8, 8, 8, None) == NO_DEVICE


def crafted_failures(st, ell, g, variant=None):
    """what a (possibly planted) restatement gets wrong on one crafted state"""
    N, G = len(st["T"]), len(st["gates"])
    rows = gr.rows(st["T"], st["C"], [0, N], st["gates"], [0, G], ell, g, variant)
    bad = []
    for i, (r, e) in enumerate(zip(rows, st["expect"])):
        if isinstance(e, str):
            bad += [] if np.isnan(r).all() else [(i, "nan", r.tolist())]
        else:
            bad += [(i,) + b for b in gr.expectation_failures(r, e)]
    fl = int(gr.flags_of(rows, [0, G], variant)[0])
    if fl & st["set"] != st["set"] or fl & st["clear"]:
        bad.append(("flags", fl, st["set"], st["clear"]))
    return bad, rows


def test_crafted_states_against_their_closed_forms(frx, sc):
    ell, g = _params(sc)
    for name, st in gs.crafted(sc.ZHANGJIAJIE).items():
        bad, rows = crafted_failures(st, ell, g)
        print(name, rows.tolist(), bad)
        assert not bad, (name, bad)
        assert np.array_equal(frx.gate_flags(rows, [0, len(rows)]), gr.flags_of(rows, [0, len(rows)])), name
        for r, e, rec in zip(rows, st["expect"], st["gates"]):             # and the sampler's formulas agree at the reported time
            if not isinstance(e, str) and r[gr.N_CROSS] > 0:
                assert not gr.field_failures(r, st["T"], st["C"], rec, ell, g), name


@pytest.mark.parametrize("variant", ["keep_tau0", "best_not_first", "no_reach", "ge_order"])
def test_planted_errors_fail_on_the_crafted_states(sc, variant):
    """keep_tau0 fails on (e) (the knot is counted twice), best_not_first on (d) (the later passage has the larger margin), no_reach on (a), (b), (g) ... (every
    margin is too large by the reach), ge_order on h_same_instant (equal times are not strictly increasing)."""
    ell, g = _params(sc)
    failing = [name for name, st in gs.crafted(sc.ZHANGJIAJIE).items() if crafted_failures(st, ell, g, variant)[0]]
    print(variant, failing)
    assert failing, f"planted error {variant!r} passes on every crafted state"


def _compare(pairs, ell, g):
    """pairs of (T (N,), Cp (N, 6, 3), record): the restatement's row against the sampler; returns (pairs, pairs left out)"""
    left_out = 0
    for i, (T, Cp, rec) in enumerate(pairs):
        row = gr.gate_row(T, Cp, rec, ell, g)
        s = gr.sample_gate(T, Cp, rec, ell, g)
        if s["doubtful"]:
            left_out += 1
            continue
        assert row[gr.N_CROSS] == s["n_cross"], (i, row.tolist(), s)
        if row[gr.N_CROSS] > 0:
            bad = gr.field_failures(row, T, Cp, rec, ell, g)
            assert not bad, (i, bad, row.tolist())
        else:
            assert row[gr.MARGIN] == -np.inf and row[gr.PIECE] == -1.0
    return len(pairs), left_out


def test_restatement_against_the_long_double_sampler_on_random_quintics(sc):
    """300 random quintics, each a candidate of one piece, with three random gates through the piece (900 pairs): N_CROSS is the sampler's count of sign changes
    over 20 001 long-double samples in physical time; at the reported TIME the long-double |n.(p - c)| <= 256 eps S, S = |c| + sum_k |c_k| T^k (Horner on
    degree 5 costs about 10 eps S, the root is bracketed to adjacent doubles against |f'| <= 5 S: under 32 eps S, times 8 for the second evaluation in
    physical time), and every other field reproduces the sampler's formula there to 1e-9 max(1, |value|).  A pair is left out only when the sampler itself sees
    a near-tangency or a root within two sample steps of a piece end; at most 2 % may be.  Observed with GATE_SEED = 5: 0 of 900 left out."""
    ell, g = _params(sc)
    rng = np.random.default_rng(GATE_SEED)
    pairs = []
    for T, c in es.random_quintics(np.random.default_rng(11), 300):
        pairs += [(np.array([T]), c[None], rec) for rec in gs.random_gates(rng, T, c, 3)]
    n, left_out = _compare(pairs, ell, g)
    print("pairs", n, "left out", left_out)
    assert n == 900 and left_out <= 0.02 * n


def test_restatement_against_the_long_double_sampler_on_optimised_candidates(sc, ob):
    """two oracle-optimised candidates (12 pieces, 3 gates each) with their own gates, framed along the polyline's bisector: the same comparison per
    (candidate, gate); every gate is crossed.  Observed: 0 of 6 left out."""
    ell, g = _params(sc)
    pairs = []
    for sid in (2, 6):
        cand = sc.make_candidate(sid, 12, 3)
        r = ob.Oracle(cand, sc.ZHANGJIAJIE, qd_intervals=8).optimize(1e-6, max_iterations=80)
        T, Cp = np.asarray(r["T"]), np.asarray(r["C"]).reshape(-1, 6, 3)
        pairs += [(T, Cp, rec) for rec in gs.candidate_gates(cand)]
    n, left_out = _compare(pairs, ell, g)
    print("pairs", n, "left out", left_out)
    assert n == 6 and left_out <= 0.02 * n
    for T, Cp, rec in pairs:
        assert gr.gate_row(T, Cp, rec, ell, g)[gr.N_CROSS] >= 1
