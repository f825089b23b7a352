"""The blocking entries that take (T, C) from the host share one staging path (fast-racing_amd/csrc/frx_handle.hpp: stage_TC, fetch_rows), one set of pinned
buffers on the handle and - the check, the extrema and the containment - one buffer of piece rows (d_rows, frx_traj.cpp).  Eleven calls in a row on ONE
handle, each with its own (T, C), must give, bit for bit, what the same call gives on a fresh handle: nothing of a call - its durations, its coefficients,
its rows - reaches the next one.  Wide rows (extrema, 10 fields) come before narrow ones (contain, check: 8) and after them, where a stale row in the shared
buffer would show.  The partials of the exact clearance stay what they were while the entries behind it run: its counts are read twice."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PIECES = (2, 5, 3)
INTERVALS, POINTS, SAMPLES = 8, 5, 7
BOX = np.concatenate([np.vstack([np.eye(3), np.diag([2.0, 2.0, 4.0])]), np.vstack([-np.eye(3), np.diag([-2.0, -2.0, 0.0])])], axis=1)
ORDER = ("check", "sample", "extrema", "contain", "clearance", "clearance_exact", "gates", "map_distance", "penalty", "extrema", "check")
EXACT_AT = ORDER.index("clearance_exact")


def handle(frx, sc):
    P = int(np.sum(PIECES))
    return frx.PenaltyProblem(sc.ZHANGJIAJIE, list(PIECES), [0] * P, [BOX], qd_intervals=8)


def state(k):
    """(T, Cf, cloud, gate corners, field) of call k: every call its own"""
    rng = np.random.default_rng(100 + k)
    P = int(np.sum(PIECES))
    T, Cf, obs = rng.uniform(0.4, 1.6, P), rng.normal(0.0, 0.6, (6 * P, 3)), rng.uniform(-2.0, 2.0, (POINTS, 3))
    # one gate per candidate: a rectangle round a random centre, in a random plane
    c = rng.uniform(-1.0, 1.0, (len(PIECES), 1, 3)); a = rng.normal(0.0, 1.0, (len(PIECES), 1, 3)); b = np.cross(a, rng.normal(0.0, 1.0, (len(PIECES), 1, 3)))
    corners = np.concatenate([c + a + b, c - a + b, c - a - b, c + a - b], axis=1)
    return T, Cf, obs, corners, rng.uniform(0.0, 3.0, 8 * 8 * 8)


def call(frx, prob, name, k):
    """the arrays call k returns, in a fixed order"""
    T, Cf, obs, corners, field = state(k)
    if name == "check":
        r = prob.trajectory_check(T, Cf, INTERVALS)
        return [r["piece"], r["candidate"], r["flags"]]
    if name == "sample":
        return [prob.trajectory_sample(T, Cf, SAMPLES)["rows"]]
    if name == "gates":
        r = prob.trajectory_gates(T, Cf, frx.gate_from_corners(corners), np.arange(len(PIECES) + 1))
        return [r["gate"], r["flags"]]
    if name == "penalty":
        return list(prob.penalty(T, Cf))
    if name == "extrema":
        r = prob.trajectory_extrema(T, Cf)
    elif name == "contain":
        r = prob.trajectory_contain(T, Cf)
    elif name == "clearance":
        r = prob.trajectory_clearance(T, Cf, obs, INTERVALS)
    elif name == "clearance_exact":
        r = prob.trajectory_clearance_exact(T, Cf, obs)
    else:
        assert name == "map_distance"
        r = prob.trajectory_map_distance(T, Cf, frx.VoxelMap([-2.0, -2.0, 0.0], [8, 8, 8], 0.5), field, 0.1, INTERVALS)
    return [r["piece"], r["cand"], r["flags"]]


def same_bits(a, b):
    a = np.ascontiguousarray(a); b = np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def test_calls_in_a_row_equal_the_calls_alone(frx, sc):
    shared = handle(frx, sc)
    try:
        got = [call(frx, shared, name, k) for k, name in enumerate(ORDER[:EXACT_AT + 1])]
        counts = shared.clear_exact_counts()                                  # straight after the exact call ...
        got += [call(frx, shared, name, EXACT_AT + 1 + k) for k, name in enumerate(ORDER[EXACT_AT + 1:])]
        counts_later = shared.clear_exact_counts()                            # ... and after gates, map_distance, penalty, extrema and check on the handle
    finally:
        shared.close()
    for k, name in enumerate(ORDER):
        fresh = handle(frx, sc)
        try:
            want = call(frx, fresh, name, k)
        finally:
            fresh.close()
        assert len(got[k]) == len(want)
        for i, (a, b) in enumerate(zip(got[k], want)):
            assert same_bits(a, b), (k, name, i, a, b)
    # the two checks and the two extrema had different inputs and so different rows: a stale row would have shown
    assert not same_bits(got[0][0], got[10][0]) and not same_bits(got[2][0], got[9][0])
    assert got[2][0].shape[1] == 10 and got[3][0].shape[1] == got[10][0].shape[1] == 8    # wide, then narrow, then wide and narrow again
    for a, b in zip(counts, counts_later):
        assert same_bits(a, b), (counts, counts_later)
    assert counts[0].sum() >= 1                                               # and they are counts: something survived the cull
