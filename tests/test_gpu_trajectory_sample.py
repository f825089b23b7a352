"""frx_trajectory_sample on the device against the numpy restatement (tests/sample_reference.py) and against the feasibility check it complements."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sample_reference as sr  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = 1e-12
NONQ = [f for f in range(20) if not 13 <= f < 17]                     # every field but the quaternion
G = 9.81                                                              # grav_acc of every handle here (scenario.ZHANGJIAJIE)


def close(a, b):
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    return np.abs(a - b) <= TOL * np.maximum(1.0, np.abs(b))


_hip = None


def hip():
    """The HIP runtime libfrx.so itself uses (torch brings a second runtime that must not be loaded after the library)."""
    global _hip
    if _hip is None:
        _hip = C.CDLL("libamdhip64.so.7")
        for name in ("hipMalloc", "hipMemcpy", "hipFree", "hipStreamCreate", "hipStreamDestroy", "hipStreamSynchronize", "hipStreamBeginCapture",
                     "hipStreamEndCapture", "hipGraphGetNodes", "hipGraphInstantiate", "hipGraphLaunch", "hipGraphExecDestroy", "hipGraphDestroy",
                     "hipDeviceSynchronize", "hipMemset"):
            getattr(_hip, name).restype = C.c_int
        _hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        _hip.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
        _hip.hipStreamBeginCapture.argtypes = [C.c_void_p, C.c_int]
        _hip.hipStreamEndCapture.argtypes = [C.c_void_p, C.c_void_p]
        _hip.hipGraphGetNodes.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        _hip.hipGraphInstantiate.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
        _hip.hipGraphLaunch.argtypes = [C.c_void_p, C.c_void_p]
        for name in ("hipStreamDestroy", "hipStreamSynchronize", "hipGraphExecDestroy", "hipGraphDestroy", "hipFree"):
            getattr(_hip, name).argtypes = [C.c_void_p]
    return _hip


class DevBuf:
    def __init__(self, host):
        host = np.ascontiguousarray(host)
        self.n = host.nbytes
        self.ptr = C.c_void_p()
        assert hip().hipMalloc(C.byref(self.ptr), C.c_size_t(self.n)) == 0
        assert hip().hipMemcpy(self.ptr, host.ctypes.data, self.n, 1) == 0              # hipMemcpyHostToDevice

    @property
    def p(self):
        return self.ptr.value

    def get(self, like):
        out = np.empty_like(like)
        assert hip().hipDeviceSynchronize() == 0
        assert hip().hipMemcpy(out.ctypes.data, self.ptr, self.n, 2) == 0               # hipMemcpyDeviceToHost
        return out

    def close(self):
        if self.ptr:
            hip().hipFree(self.ptr)
            self.ptr = None


def assert_rows(got, ref):
    """Every field but the quaternion to TOL (NaN exactly where the restatement has NaN); the quaternion through its rotation matrix, and component
    by component where w > 1e-6 (below that its sign is a matter of rounding)."""
    assert got.shape == ref.shape
    g, r = got[..., NONQ], ref[..., NONQ]
    assert np.array_equal(np.isnan(g), np.isnan(r))
    # the body rates are projections of j / |h| (over |(0, zB.z, -zB.y)| for omega_z): they round relative to that size, not to their own
    with np.errstate(invalid="ignore", divide="ignore"):
        thr, _, m = sr.frame(ref[..., 6:9].reshape(-1, 3), G)
        size = (np.linalg.norm(ref[..., 9:12].reshape(-1, 3), axis=1) / thr / m).reshape(ref.shape[:-1])
    scale = np.maximum(1.0, np.abs(r))
    scale[..., -3:] = np.fmax(scale[..., -3:], size[..., None])
    ok = (np.abs(g - r) <= TOL * scale) | np.isnan(r)
    assert ok.all(), (np.argwhere(~ok)[:5], g[~ok][:5], r[~ok][:5])
    qg, qr = got[..., 13:17].reshape(-1, 4), ref[..., 13:17].reshape(-1, 4)
    fin = np.isfinite(qr).all(axis=1)
    assert np.array_equal(fin, np.isfinite(qg).all(axis=1))
    assert np.abs(sr.quat_to_R(qg[fin]) - sr.quat_to_R(qr[fin])).max(initial=0.0) <= TOL
    pos = fin & (qr[:, 0] > 1e-6)
    assert close(qg[pos], qr[pos]).all()


def special_times(T, piece_off, S, rng):
    """(B, S) times: every interior knot, before the start, the start, the end, past the end, NaN, the rest uniform over the duration."""
    B = len(piece_off) - 1
    times = np.empty((B, S))
    for b in range(B):
        cum = sr.prefix_sums(T[piece_off[b]:piece_off[b + 1]])
        sp = np.concatenate([cum[1:-1], [-1.0, -0.0, 0.0, cum[-1], cum[-1] + 0.5, np.inf, -np.inf, np.nan]])
        assert len(sp) <= S
        times[b] = np.concatenate([sp, rng.uniform(0.0, cum[-1], S - len(sp))])
    return times


@pytest.fixture(scope="module")
def headline(frx, sc):
    B, N, gates, kappa = sc.CONFIGS["headline"]
    cands = sc.make_batch(0, B, N, gates)
    prob = frx.Problem(cands, sc.ZHANGJIAJIE, qd_intervals=kappa)
    x0 = prob.initial_guess()
    T0, C0 = prob.forward(x0)
    res = prob.optimize(sc.ZHANGJIAJIE["opt_rel_tol"], x0=x0)
    states = {"initial": (T0, C0), "optimised": (res["T"], res["C"])}
    yield cands, prob, states
    prob.close()


@pytest.mark.parametrize("state", ["initial", "optimised"])
def test_agrees_with_numpy_on_the_headline_batch(headline, sc, state):
    cands, prob, states = headline
    T, Cf = states[state]
    rng = np.random.default_rng(7)
    S = 700
    times = special_times(T, prob.piece_off, S, rng)
    for kw in (dict(), dict(dt=1e-3), dict(dt=0.0137, t0=-0.3), dict(times=times)):
        got = prob.trajectory_sample(T, Cf, S, **kw)
        assert got["rows"].shape == (prob.B, S, 20) and got["rows"].dtype == np.float64
        assert_rows(got["rows"], sr.sample_batch(T, Cf, prob.piece_off, S, G, **kw))
        assert np.shares_memory(got["quat"], got["rows"]) and got["thrust"].shape == (prob.B, S) and got["omega"].shape == (prob.B, S, 3)
    got = prob.trajectory_sample(T, Cf, S, times=times)["rows"]
    assert np.isnan(got[:, 63 + 7]).all() and np.isfinite(got[:, :63 + 7]).all()                 # (headline: 64 pieces, 63 interior knots)
    assert np.array_equal(got[:, 63], got[:, 65]) and np.array_equal(got[:, 66], got[:, 68])      # before the start = start, past the end = end


def test_ragged_batch(frx, sc):
    """Candidates of 1 to 128 pieces (a PenaltyProblem handle: random quintics over given durations)."""
    counts = [1, 3, 17, 64, 65, 100, 128, 7]
    box = np.concatenate([np.vstack([np.eye(3), 1e3 * np.ones((3, 3))]), np.vstack([-np.eye(3), -1e3 * np.ones((3, 3))])], axis=1)
    prob = frx.PenaltyProblem(sc.ZHANGJIAJIE, counts, [0] * sum(counts), [box], qd_intervals=8)
    assert list(np.diff(prob.piece_off)) == counts
    rng = np.random.default_rng(11)
    T = rng.uniform(0.05, 0.4, prob.P)
    Cf = rng.normal(0.0, 2.0, (6 * prob.P, 3))
    S = 300
    times = special_times(T, prob.piece_off, S, rng)
    for kw in (dict(), dict(dt=2.5e-3), dict(times=times)):
        assert_rows(prob.trajectory_sample(T, Cf, S, **kw)["rows"], sr.sample_batch(T, Cf, prob.piece_off, S, G, **kw))
    prob.close()


def test_consistent_with_the_check(headline):
    """Every piece sampled at cum[i] + j T_i / M through `times`: the maxima of |v|, |a|, |omega_xy| and the range of |h| are the check's at M."""
    cands, prob, states = headline
    T, Cf = states["optimised"]
    M = 64
    chk = prob.trajectory_check(T, Cf, M)
    per = prob.piece_off
    N = int(np.diff(per).max())
    times = np.full((prob.B, N * (M + 1)), np.nan)
    for b in range(prob.B):
        t = T[per[b]:per[b + 1]]
        cum = sr.prefix_sums(t)
        tb = np.concatenate([cum[i] + (t[i] / M) * np.arange(M + 1) for i in range(len(t))])
        times[b, :len(tb)] = tb
        times[b, len(tb):] = tb[-1]
    rows = prob.trajectory_sample(T, Cf, times.shape[1], times=times)["rows"]
    speed = np.linalg.norm(rows[..., 3:6], axis=2).max(axis=1)
    acc = np.linalg.norm(rows[..., 6:9], axis=2).max(axis=1)
    bdr = np.linalg.norm(rows[..., 17:19], axis=2).max(axis=1)
    for got, want in ((speed, chk["speed"]), (acc, chk["acc"]), (bdr, chk["body_rate"]), (rows[..., 12].min(axis=1), chk["thrust_min"]),
                      (rows[..., 12].max(axis=1), chk["thrust_max"])):
        assert close(got, want).all(), (got[:4], want[:4])


def test_continuous_across_knots(headline):
    """p, v, a, j at a knot (the earlier piece's end) and just after it (the later piece's start) agree."""
    cands, prob, states = headline
    for state in ("initial", "optimised"):
        T, Cf = states[state]
        per = prob.piece_off
        N = int(np.diff(per).max())
        times = np.empty((prob.B, 2 * (N - 1)))
        for b in range(prob.B):
            knots = sr.prefix_sums(T[per[b]:per[b + 1]])[1:-1]
            times[b, 0::2] = knots
            times[b, 1::2] = np.nextafter(knots, np.inf)
        rows = prob.trajectory_sample(T, Cf, times.shape[1], times=times)["rows"][..., :12]
        a, b = rows[:, 0::2], rows[:, 1::2]
        err = np.abs(a - b) / np.maximum(1.0, np.abs(a))
        assert err.max() <= 1e-8, (state, err.max(), np.unravel_index(np.argmax(err), err.shape))


def test_forms_determinism_and_isolation(frx, sc, headline):
    cands, prob, states = headline
    T, Cf = states["optimised"]
    S = 1000
    a = prob.trajectory_sample(T, Cf, S, dt=1e-3)["rows"]
    b = prob.trajectory_sample(T, Cf, S, dt=1e-3)["rows"]
    assert np.array_equal(a, b)
    host = np.full(prob.B * S * 20, -7.0)
    Td, Cd, out = DevBuf(T), DevBuf(np.ascontiguousarray(Cf).reshape(-1)), DevBuf(host)
    prob.trajectory_sample_device(Td.p, Cd.p, out.p, S, dt=1e-3)
    assert np.array_equal(out.get(host).reshape(prob.B, S, 20), a)
    times = special_times(T, prob.piece_off, S, np.random.default_rng(1))
    tdev = DevBuf(times)
    prob.trajectory_sample_device(Td.p, Cd.p, out.p, S, times_ptr=tdev.p)
    assert np.array_equal(out.get(host).reshape(prob.B, S, 20), prob.trajectory_sample(T, Cf, S, times=times)["rows"], equal_nan=True)
    # a misaligned output is refused, nothing is launched
    with pytest.raises(frx.FrxError):
        prob.trajectory_sample_device(Td.p, Cd.p, out.p + 8, S, dt=1e-3)
    for d in (Td, Cd, out, tdev):
        d.close()
    for q in (0, 7, len(cands) - 1):
        sl = slice(prob.piece_off[q], prob.piece_off[q + 1])
        solo = frx.Problem([cands[q]], sc.ZHANGJIAJIE, qd_intervals=prob.kappa)
        assert np.array_equal(solo.trajectory_sample(T[sl], Cf[6 * sl.start:6 * sl.stop], S, dt=1e-3)["rows"][0], a[q])
        solo.close()
    # NaN in one candidate's coefficients, NaN in another's duration: every other candidate's rows are untouched
    clean = prob.trajectory_sample(T, Cf, S)["rows"]
    bad_C = np.array(Cf, copy=True); bad_T = np.array(T, copy=True)
    bad_C[6 * (prob.piece_off[3] + 5) + 2, 1] = np.nan
    bad_T[prob.piece_off[9] + 20] = np.nan
    got = prob.trajectory_sample(bad_T, bad_C, S)["rows"]
    keep = np.setdiff1d(np.arange(prob.B), [3, 9])
    assert np.array_equal(got[keep], clean[keep])
    assert np.isnan(got[3]).any() and np.isfinite(got[3, 0]).all() and np.isnan(got[9]).all()     # (9: its duration is NaN, so is every time)


def test_graph_capture(headline):
    """The device form is a pure launch: captured on a caller stream it is one kernel node, and replaying the graph gives the same bits."""
    cands, prob, states = headline
    T, Cf = states["optimised"]
    S = 512
    want = prob.trajectory_sample(T, Cf, S, dt=2e-3, t0=0.1)["rows"]
    host = np.zeros(prob.B * S * 20)
    Td, Cd, out = DevBuf(T), DevBuf(np.ascontiguousarray(Cf).reshape(-1)), DevBuf(host)
    H = hip()
    st, graph, exe, n = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_size_t(0)
    assert H.hipStreamCreate(C.byref(st)) == 0
    try:
        assert H.hipStreamBeginCapture(st, 0) == 0                                         # hipStreamCaptureModeGlobal
        prob.trajectory_sample_device(Td.p, Cd.p, out.p, S, dt=2e-3, t0=0.1, stream=st.value)
        assert H.hipStreamEndCapture(st, C.byref(graph)) == 0
        assert H.hipGraphGetNodes(graph, None, C.byref(n)) == 0 and n.value == 1
        assert H.hipGraphInstantiate(C.byref(exe), graph, None, None, 0) == 0
        for _ in range(2):
            assert H.hipMemset(out.ptr, 0, out.n) == 0
            assert H.hipGraphLaunch(exe, st) == 0 and H.hipStreamSynchronize(st) == 0
            assert np.array_equal(out.get(host).reshape(prob.B, S, 20), want)
    finally:
        if exe.value:
            H.hipGraphExecDestroy(exe)
        if graph.value:
            H.hipGraphDestroy(graph)
        H.hipStreamDestroy(st)
        for d in (Td, Cd, out):
            d.close()


def test_monte_carlo_share(frx, sc):
    B, N, gates, kappa = sc.CONFIGS["montecarlo4096"]
    B //= 8                                                             # one GPU's share, as bench.py quotes it
    cands = [sc.make_candidate(b, N, gates) for b in range(B)]
    prob = frx.Problem(cands, sc.ZHANGJIAJIE, qd_intervals=kappa)
    T, Cf = prob.forward(prob.initial_guess())
    S = 4096
    rows = prob.trajectory_sample(T, Cf, S)["rows"]
    assert rows.shape == (B, S, 20) and np.isfinite(rows).all()
    pick = sorted(np.random.default_rng(5).choice(B, 12, replace=False))
    assert_rows(rows[pick], sr.sample_batch(T, Cf, prob.piece_off, S, G, cands=pick))
    prob.close()


def test_argument_errors_on_a_real_handle(frx, headline):
    cands, prob, states = headline
    T, Cf = states["optimised"]
    L = frx.lib()
    out = np.zeros(prob.B * 4 * 20)
    t, c = np.ascontiguousarray(T), np.ascontiguousarray(Cf).reshape(-1)
    for S, t0, dt in ((0, 0.0, 1e-3), (1, 0.0, 0.0), (4, 0.0, -1e-3), (4, np.nan, 1e-3), (4, 0.0, np.inf)):
        assert L.frx_trajectory_sample(prob.h, t.ctypes.data, c.ctypes.data, S, t0, dt, None, out.ctypes.data) == -1
    assert not out.any()
    # more than the device holds: FRX_ERR_ALLOC before anything is copied or launched, and the handle stays usable
    assert L.frx_trajectory_sample(prob.h, t.ctypes.data, c.ctypes.data, 2 ** 31 - 1, 0.0, 1e-3, None, out.ctypes.data) == -6
    assert not out.any()
    assert np.isfinite(prob.trajectory_sample(T, Cf, 4, dt=1e-3)["rows"]).all()
    with pytest.raises(ValueError):
        prob.trajectory_sample(T, Cf, 4, times=np.zeros((prob.B, 5)))
