"""frx_trajectory_check on the device against the numpy restatement (tests/check_reference.py) and against the penalty it complements."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import check_reference as cr  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = 1e-12


def close(a, b):
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    return np.abs(a - b) <= TOL * np.maximum(1.0, np.abs(b))


class DevBuf:
    """Device memory through the HIP runtime libfrx.so itself uses (torch brings a second runtime that must not be loaded after the library)."""
    _hip = None

    def __init__(self, host):
        import ctypes as C
        if DevBuf._hip is None:
            DevBuf._hip = C.CDLL("libamdhip64.so.7")
        self.n = host.nbytes
        self.ptr = C.c_void_p()
        assert DevBuf._hip.hipMalloc(C.byref(self.ptr), C.c_size_t(self.n)) == 0
        assert DevBuf._hip.hipMemcpy(self.ptr, C.c_void_p(host.ctypes.data), C.c_size_t(self.n), 1) == 0     # hipMemcpyHostToDevice

    def get(self, like):
        import ctypes as C
        out = np.empty_like(like)
        assert DevBuf._hip.hipDeviceSynchronize() == 0
        assert DevBuf._hip.hipMemcpy(C.c_void_p(out.ctypes.data), self.ptr, C.c_size_t(self.n), 2) == 0       # hipMemcpyDeviceToHost
        return out

    def close(self):
        if self.ptr:
            DevBuf._hip.hipFree(self.ptr)
            self.ptr = None


def piece_polys(cands):
    # gridRes = inf (ZHANGJIAJIE): one fine piece per corridor cell, in candidate order
    return [h for c in cands for h in c.h_polys]


@pytest.fixture(scope="module")
def headline(frx, sc):
    B, N, gates, kappa = sc.CONFIGS["headline"]
    cands = sc.make_batch(0, B, N, gates)
    prob = frx.Problem(cands, sc.ZHANGJIAJIE, qd_intervals=kappa)
    assert prob.P == prob.Pc
    x0 = prob.initial_guess()
    T0, C0 = prob.forward(x0)
    res = prob.optimize(sc.ZHANGJIAJIE["opt_rel_tol"], x0=x0)
    states = {"initial": (T0, C0), "optimised": (res["T"], res["C"])}
    yield cands, prob, states
    prob.close()


def assert_agrees(got, T, Cf, polys, params, M, piece_off):
    ref = cr.check_pieces(T, Cf, polys, params, M)
    ok = close(got["piece"][:, :6], ref[:, :6])
    assert ok.all(), (M, np.argwhere(~ok)[:5], got["piece"][~ok.all(axis=1)][:2], ref[~ok.all(axis=1)][:2])
    # the reported worst sample attains the maximum: recompute it where the device says it is
    ell, g = cr.params_of(params)
    Cp = np.asarray(Cf).reshape(-1, 6, 3)
    for i in range(len(T)):
        step = T[i] / M
        j = int(round(got["piece"][i, 6] / step)); k = int(got["piece"][i, 7])
        assert 0 <= j <= M and got["piece"][i, 6] == step * j, (i, got["piece"][i, 6:])
        v = cr.piece_samples(Cp[i], float(T[i]), M, polys[i], ell, g)["corridor"]
        assert 0 <= k < v.shape[1] and abs(v[j, k] - ref[i, 0]) <= TOL * max(1.0, abs(ref[i, 0])), (i, j, k, v[j, k], ref[i, 0])
    cref = cr.reduce_candidates(ref, T, piece_off)
    assert close(got["candidate"][:, :6], cref[:, :6]).all()
    for b in range(len(piece_off) - 1):
        q = piece_off[b] + int(got["candidate"][b, 7])
        assert abs(ref[q, 0] - cref[b, 0]) <= TOL * max(1.0, abs(cref[b, 0]))
        assert abs(got["candidate"][b, 6] - (np.sum(T[piece_off[b]:q]) + got["piece"][q, 6])) <= TOL * max(1.0, got["candidate"][b, 6])
    assert np.array_equal(got["flags"], cr.flags_of(cref, params)), (got["flags"], cr.flags_of(cref, params))
    return ref


@pytest.mark.parametrize("state", ["initial", "optimised"])
def test_agrees_with_numpy_on_the_headline_batch(headline, sc, state):
    cands, prob, states = headline
    T, Cf = states[state]
    polys = piece_polys(cands)
    for M in (1, 16, 31, 63, 64, 256, 1000):
        got = prob.trajectory_check(T, Cf, M)
        assert_agrees(got, T, Cf, polys, sc.ZHANGJIAJIE, M, prob.piece_off)
        assert got["piece"].shape == (prob.P, 8) and got["candidate"].shape == (prob.B, 8) and got["flags"].dtype == np.uint32
        assert np.array_equal(got["speed"], got["candidate"][:, 1])


@pytest.mark.parametrize("state", ["initial", "optimised"])
def test_consistent_with_the_penalty_at_its_nodes(headline, sc, state):
    """At M = kappa the check samples the penalty's nodes: a piece is violated there exactly when its penalty cost is positive."""
    cands, prob, states = headline
    T, Cf = states[state]
    p = sc.ZHANGJIAJIE
    rows = prob.trajectory_check(T, Cf, prob.kappa)["piece"]
    host = np.zeros(prob.P * 20)
    Td, Cd, out = DevBuf(np.ascontiguousarray(T)), DevBuf(np.ascontiguousarray(Cf).reshape(-1)), DevBuf(host)
    prob.penalty_device(Td.ptr.value, Cd.ptr.value, out.ptr.value, 0)
    cost = out.get(host).reshape(-1, 20)[:, 0]
    for d in (Td, Cd, out):
        d.close()
    violated = ((rows[:, 0] + p["safe_margin"] > 0) | (rows[:, 1] > p["vel_max"]) | (rows[:, 2] < p["thr_acc_min"]) | (rows[:, 3] > p["thr_acc_max"])
                | (rows[:, 4] > p["body_rate_max"]))
    assert np.array_equal(violated, cost > 0), (np.argwhere(violated != (cost > 0))[:5], violated.sum(), (cost > 0).sum())


def test_violation_between_the_nodes(frx, sc):
    """One quintic piece that sits at the box's centre at the kappa + 1 = 5 nodes and bulges past a face between them: the penalty sees nothing,
    the dense check sees the bulge where numpy puts it."""
    params = dict(sc.ZHANGJIAJIE)
    params.update(vel_max=1e4, thr_acc_min=0.0, thr_acc_max=1e6, body_rate_max=1e6)
    # faces x <= 2, y <= 2, z <= 4, x >= -2, y >= -2, z >= 0 as columns (outer normal, point)
    box = np.concatenate([np.vstack([np.eye(3), np.diag([2.0, 2.0, 4.0])]), np.vstack([-np.eye(3), np.diag([-2.0, -2.0, 0.0])])], axis=1)
    prob = frx.PenaltyProblem(params, [1], [0], [box], qd_intervals=4)
    T = np.array([1.0])
    Cf = np.zeros((6, 3))
    Cf[0] = (0.3, 0.0, 2.0)                                             # (off centre along x: the bulge towards x <= 2 is the larger of the two)
    Cf[:, 0] += 1000.0 * np.poly([0.0, 0.25, 0.5, 0.75, 1.0])[::-1]     # x - 0.3 = A prod (s - j/4): zero at the nodes, about 3.5 m in between
    cost, _, _ = prob.penalty(T, Cf)
    assert cost[0] == 0.0
    got = prob.trajectory_check(T, Cf, 64)
    assert got["flags"][0] & frx.CHECK_FLAG_CORRIDOR and got["corridor"][0] > 1.0
    ell, g = cr.params_of(params)
    dense = cr.piece_samples(Cf, 1.0, 1 << 14, box, ell, g)
    t_np = dense["s"][np.argmax(dense["corridor"].max(axis=1))]
    assert abs(got["worst_t"][0] - t_np) <= 1.0 / 64, (got["worst_t"][0], t_np)
    assert_agrees(got, T, Cf, [box], params, 64, [0, 1])
    prob.close()


def test_deterministic_and_independent_of_the_batch(frx, sc, headline):
    cands, prob, states = headline
    T, Cf = states["optimised"]
    M = 256
    a = prob.trajectory_check(T, Cf, M); b = prob.trajectory_check(T, Cf, M)
    for k in ("piece", "candidate", "flags"):
        assert np.array_equal(a[k], b[k], equal_nan=True)
    host = np.full(prob.P * 8, -7.0)
    Td, Cd, out = DevBuf(np.ascontiguousarray(T)), DevBuf(np.ascontiguousarray(Cf).reshape(-1)), DevBuf(host)
    prob.trajectory_check_device(Td.ptr.value, Cd.ptr.value, out.ptr.value, M, 0)
    assert np.array_equal(out.get(host).reshape(-1, 8), a["piece"])
    for d in (Td, Cd, out):
        d.close()
    for q in (0, 7, len(cands) - 1):
        sl = slice(prob.piece_off[q], prob.piece_off[q + 1])
        solo = frx.Problem([cands[q]], sc.ZHANGJIAJIE, qd_intervals=prob.kappa)
        r = solo.trajectory_check(T[sl], Cf[6 * sl.start:6 * sl.stop], M)
        assert np.array_equal(r["piece"], a["piece"][sl]) and np.array_equal(r["candidate"][0], a["candidate"][q]) and r["flags"][0] == a["flags"][q]
        solo.close()


def test_nan_propagates_to_its_piece_only(headline):
    cands, prob, states = headline
    T, Cf = states["optimised"]
    clean = prob.trajectory_check(T, Cf, 64)
    q = prob.piece_off[3] + 5
    bad = np.array(Cf, copy=True)
    bad[6 * q + 5, 0] = np.nan
    got = prob.trajectory_check(T, bad, 64)
    assert np.isnan(got["piece"][q, :6]).all()
    others = np.arange(prob.P) != q
    assert np.array_equal(got["piece"][others], clean["piece"][others])
    assert got["flags"][3] & 32 and np.isnan(got["candidate"][3, :6]).all() and got["candidate"][3, 7] == 5
    keep = np.arange(prob.B) != 3
    assert np.array_equal(got["candidate"][keep], clean["candidate"][keep]) and np.array_equal(got["flags"][keep], clean["flags"][keep])


def test_monte_carlo_share(frx, sc):
    B, N, gates, kappa = sc.CONFIGS["montecarlo4096"]
    B //= 8                                                             # one GPU's share, as bench.py quotes it
    cands = [sc.make_candidate(b, N, gates) for b in range(B)]
    prob = frx.Problem(cands, sc.ZHANGJIAJIE, qd_intervals=kappa)
    T, Cf = prob.forward(prob.initial_guess())
    got = prob.trajectory_check(T, Cf, 256)
    assert np.isfinite(got["piece"]).all()
    rng = np.random.default_rng(5)
    for b in sorted(rng.choice(B, 16, replace=False)):
        sl = slice(prob.piece_off[b], prob.piece_off[b + 1])
        sub = dict(piece=got["piece"][sl], candidate=got["candidate"][b:b + 1], flags=got["flags"][b:b + 1])
        assert_agrees(sub, T[sl], Cf[6 * sl.start:6 * sl.stop], cands[b].h_polys, sc.ZHANGJIAJIE, 256, [0, sl.stop - sl.start])
    prob.close()
