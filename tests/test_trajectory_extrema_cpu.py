"""The restatement of frx_trajectory_extrema (tests/extrema_reference.py) against the host's frx_traj_max_rates, against an independent long-double
sampler, and with planted errors - no device needed.  The device kernel is held to the restatement bit for bit in tests/test_gpu_trajectory_extrema.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import extrema_reference as er  # noqa: E402
import extrema_states as es  # noqa: E402

INVALID_ARG, NO_DEVICE = -1, -2


def _optimised(sc, ob, sid=2, N=10, gates=2):
    cand = sc.make_candidate(sid, N, gates)
    r = ob.Oracle(cand, sc.ZHANGJIAJIE, qd_intervals=8).optimize(1e-6, max_iterations=80)
    return r["T"], r["C"]


@pytest.fixture(scope="module")
def optimised(sc, ob):
    """two optimised trajectories, their restatement rows computed once and left unchanged"""
    g = sc.ZHANGJIAJIE["grav_acc"]
    out = []
    for sid in (2, 6):
        T, Cf = _optimised(sc, ob, sid, 12, 3)
        out.append((T, Cf, er.rows(T, Cf, g)))
    return out


@pytest.fixture(scope="module")
def quintics(sc):
    g = sc.ZHANGJIAJIE["grav_acc"]
    pieces = es.random_quintics(np.random.default_rng(11), 300)
    T = np.array([t for t, _ in pieces])
    Cf = np.array([c for _, c in pieces]).reshape(-1, 3)
    return T, Cf, er.rows(T, Cf, g)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_restatement_reproduces_the_host_function_bit_for_bit(frx, optimised, quintics):
    """SPEED and ACC of the restatement are frx_traj_max_rates' numbers, bit for bit, wherever that function does not take its early-out - and the inputs
    are built so that it never does (asserted, none left out)."""
    for T, Cf, ref in optimised + [quintics]:
        Cp = np.asarray(Cf).reshape(-1, 6, 3)
        for i in range(len(T)):
            dn = er.host_derivative_norms(Cp[i], T[i])
            assert min(dn) >= 2.220446049250313e-16, (i, dn)
        mv, ma = frx.traj_max_rates(T, Cf)
        assert np.array_equal(bits(mv), bits(ref[:, 0])), np.argwhere(bits(mv) != bits(ref[:, 0]))[:5]
        assert np.array_equal(bits(ma), bits(ref[:, 1])), np.argwhere(bits(ma) != bits(ref[:, 1]))[:5]


def test_constant_velocity_piece_reports_its_speed(frx, sc):
    """v = (3, -4, 0): the host function takes the reference's early-out and says 0; a certificate says 5, at time 0"""
    st = es.crafted(sc.ZHANGJIAJIE)["a_constant_velocity"]
    mv, _ = frx.traj_max_rates(np.array([st["T"]]), st["c"])
    assert mv[0] == 0.0
    row = er.piece_row(st["c"], st["T"], sc.ZHANGJIAJIE["grav_acc"])
    assert row[0] == 5.0 and row[5] == 0.0


def test_restatement_against_the_long_double_sampler(sc, optimised, quintics):
    """Every field against 20 001 long-double samples in physical time: a maximum is >= sampled (1 - 1e-12) and <= sampled (1 + 1e-6) + 1e-12 (the bounds of
    test_max_rates_bound_dense_sampling), the minimum mirrored, and every reported time reproduces its value to 1e-9 when the sampler's formula is evaluated there."""
    g = sc.ZHANGJIAJIE["grav_acc"]
    T, Cf, ref = quintics
    cases = [(t, c, r) for t, c, r in optimised] + [(T[:60], Cf[:360], ref[:60])]
    for T, Cf, ref in cases:
        Cp = np.asarray(Cf).reshape(-1, 6, 3)
        for i in range(len(T)):
            bad = er.bound_failures(ref[i], Cp[i], float(T[i]), g)
            print(i, ref[i][:5], bad)
            assert not bad, (i, bad)


def test_crafted_states_against_sampler_and_closed_form(sc):
    g = sc.ZHANGJIAJIE["grav_acc"]
    for name, st in es.crafted(sc.ZHANGJIAJIE).items():
        row = er.piece_row(st["c"], st["T"], g)
        bad = er.bound_failures(row, st["c"], st["T"], g) + er.expectation_failures(row, st["expect"])
        print(name, row, bad)
        assert not bad, (name, bad)
    f = es.crafted(sc.ZHANGJIAJIE)["f_two_equal_maxima"]
    row = er.piece_row(f["c"], f["T"], g)
    assert abs(row[5] - 0.25) < 1e-6 or abs(row[5] - 0.75) < 1e-6
    at = er.sample_values(f["c"], [0.25, 0.75], g)["speed"]
    if at[0] == at[1] and er.piece_row(f["c"], f["T"], g, "ge")[0] == row[0]:
        assert abs(row[5] - 0.25) < 1e-6                                  # equal values: the earlier candidate


@pytest.mark.parametrize("variant", ["no_end", "drop_fa", "ge", "min_first"])
def test_planted_errors_fail_on_the_crafted_states(sc, variant):
    """A restatement with a planted error - a missing end point, a dropped fa == 0 root, >= in place of >, the minimum taken from the first candidate - must
    fail the comparison of test_crafted_states_against_sampler_and_closed_form on at least one crafted state.

    no_end fails on (c) (the maximum IS the end), ge on (a) (every candidate ties: the reported time moves from 0 to T), min_first on (b) (thrust falls over the
    piece, the first candidate is its maximum).  drop_fa can fail in one way only: the fa == 0 branch of roots_unit appends a root only at tau = 0 (an interval that
    starts at a critical point a with f(a) == 0 follows one that ended there with fb == 0 and has appended a already, unless that one began with fa == 0 too - two
    exact roots with no critical point between them, which Rolle's theorem excludes), and tau = 0 is a candidate as an end as well, so no value changes; what
    changes is the ORDER of the candidates, and with it which of two equal ones is named.  State (k) has equal maxima at both ends, both exact roots: the rule names
    time 0, the planted error names T."""
    g = sc.ZHANGJIAJIE["grav_acc"]
    failing = []
    for name, st in es.crafted(sc.ZHANGJIAJIE).items():
        row = er.piece_row(st["c"], st["T"], g, variant)
        bad = er.bound_failures(row, st["c"], st["T"], g) + er.expectation_failures(row, st["expect"])
        print(variant, name, bad)
        if bad:
            failing.append(name)
    assert failing, f"planted error {variant!r} passes the comparison on every crafted state"


def test_argument_errors_come_before_the_device(frx):
    L = frx.lib()
    h = 8                                                                # never read: the NULL checks come first
    assert L.frx_trajectory_extrema(None, 8, 8, 8, 8, 8) == INVALID_ARG
    assert L.frx_trajectory_extrema(h, None, 8, 8, 8, 8) == INVALID_ARG
    assert L.frx_trajectory_extrema(h, 8, None, 8, 8, 8) == INVALID_ARG
    assert L.frx_trajectory_extrema(h, 8, 8, 8, None, 8) == INVALID_ARG
    assert L.frx_trajectory_extrema_device(None, 8, 8, 8, None) == INVALID_ARG
    assert L.frx_trajectory_extrema_device(h, 8, 8, None, None) == INVALID_ARG
    if L.frx_device_count() < 1:
        assert L.frx_trajectory_extrema(h, 8, 8, None, 8, None) == NO_DEVICE
        assert L.frx_trajectory_extrema_device(h, 8, 8, 8, None) == NO_DEVICE
