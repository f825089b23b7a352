"""The blocking entries that take (T, C) from the host share one staging path (fast-racing_amd/csrc/frx_api.cpp: stage_TC, fetch_rows) and one set of pinned
buffers on the handle.  Six calls in a row on ONE handle, each with its own (T, C), must give, bit for bit, what the same call gives on a fresh handle:
nothing of a call - its durations, its coefficients, its rows - reaches the next one."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PIECES = (2, 5, 3)
INTERVALS, POINTS, SAMPLES = 8, 5, 7
BOX = np.concatenate([np.vstack([np.eye(3), np.diag([2.0, 2.0, 4.0])]), np.vstack([-np.eye(3), np.diag([-2.0, -2.0, 0.0])])], axis=1)
ORDER = ("check", "sample", "extrema", "clearance", "penalty", "check")


def handle(frx, sc):
    P = int(np.sum(PIECES))
    return frx.PenaltyProblem(sc.ZHANGJIAJIE, list(PIECES), [0] * P, [BOX], qd_intervals=8)


def state(k):
    """(T, Cf, cloud) of call k: every call its own"""
    rng = np.random.default_rng(100 + k)
    P = int(np.sum(PIECES))
    return rng.uniform(0.4, 1.6, P), rng.normal(0.0, 0.6, (6 * P, 3)), rng.uniform(-2.0, 2.0, (POINTS, 3))


def call(prob, name, k):
    """the arrays call k returns, in a fixed order"""
    T, Cf, obs = state(k)
    if name == "check":
        r = prob.trajectory_check(T, Cf, INTERVALS)
        return [r["piece"], r["candidate"], r["flags"]]
    if name == "sample":
        return [prob.trajectory_sample(T, Cf, SAMPLES)["rows"]]
    if name == "extrema":
        r = prob.trajectory_extrema(T, Cf)
        return [r["piece"], r["cand"], r["flags"]]
    if name == "clearance":
        r = prob.trajectory_clearance(T, Cf, obs, INTERVALS)
        return [r["piece"], r["cand"], r["flags"]]
    return list(prob.penalty(T, Cf))


def same_bits(a, b):
    a = np.ascontiguousarray(a); b = np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def test_calls_in_a_row_equal_the_calls_alone(frx, sc):
    shared = handle(frx, sc)
    try:
        got = [call(shared, name, k) for k, name in enumerate(ORDER)]
    finally:
        shared.close()
    for k, name in enumerate(ORDER):
        fresh = handle(frx, sc)
        try:
            want = call(fresh, name, k)
        finally:
            fresh.close()
        assert len(got[k]) == len(want)
        for i, (a, b) in enumerate(zip(got[k], want)):
            assert same_bits(a, b), (k, name, i, a, b)
    # the two checks had different inputs and so different rows: a stale row would have shown
    assert not same_bits(got[0][0], got[5][0])
