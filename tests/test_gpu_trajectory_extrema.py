"""frx_trajectory_extrema on the device: bit for bit against the float64 restatement (tests/extrema_reference.py), against the host's frx_traj_max_rates and
the reference's recorded maxima, against the sampling check it complements, and on the crafted states of tests/extrema_states.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import extrema_reference as er  # noqa: E402
import extrema_states as es  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = 1e-12                                                             # tests/test_gpu_trajectory_check.py's own
KAPPA = es.KAPPA
BOX = np.concatenate([np.vstack([np.eye(3), np.diag([2.0, 2.0, 4.0])]), np.vstack([-np.eye(3), np.diag([-2.0, -2.0, 0.0])])], axis=1)
LAYOUTS = [(1,), (1, 5, 57), (1, 5, 58), (1, 6, 58), (1, 64, 64)]      # P = 1, 63, 64, 65, 129: the wave and workgroup edges


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def differ(a, b):
    """where two arrays differ as uint64; two values that are both not a number count as equal (which NaN a 0 / 0 yields is the machine's business)"""
    a = np.ascontiguousarray(a, dtype=np.float64); b = np.ascontiguousarray(b, dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return np.argwhere((bits(a) != bits(b)) & ~(np.isnan(a) & np.isnan(b)))


def same(a, b):
    return len(differ(a, b)) == 0


class DevBuf:
    """Device memory through the HIP runtime libfrx.so itself uses"""
    _hip = None

    def __init__(self, host):
        if DevBuf._hip is None:
            DevBuf._hip = C.CDLL("libamdhip64.so.7")
        self.n = host.nbytes
        self.ptr = C.c_void_p()
        assert DevBuf._hip.hipMalloc(C.byref(self.ptr), C.c_size_t(self.n)) == 0
        assert DevBuf._hip.hipMemcpy(self.ptr, C.c_void_p(host.ctypes.data), C.c_size_t(self.n), 1) == 0

    def get(self, like):
        out = np.empty_like(like)
        assert DevBuf._hip.hipDeviceSynchronize() == 0
        assert DevBuf._hip.hipMemcpy(C.c_void_p(out.ctypes.data), self.ptr, C.c_size_t(self.n), 2) == 0
        return out

    def close(self):
        if self.ptr:
            DevBuf._hip.hipFree(self.ptr)
            self.ptr = None


def penalty_handle(frx, sc, piece_n):
    P = int(np.sum(piece_n))
    return frx.PenaltyProblem(sc.ZHANGJIAJIE, list(piece_n), [0] * P, [BOX], qd_intervals=KAPPA)


@pytest.fixture(scope="module")
def pool(frx, sc):
    """130 pieces of two candidates at the initial guess and after a short optimisation, with their restatement rows: computed once, shared, left unchanged"""
    g = sc.ZHANGJIAJIE["grav_acc"]
    cands = sc.make_batch(0, 2, 65, 16)
    prob = frx.Problem(cands, sc.ZHANGJIAJIE, qd_intervals=KAPPA)
    x0 = prob.initial_guess()
    T0, C0 = prob.forward(x0)
    res = prob.optimize(sc.ZHANGJIAJIE["opt_rel_tol"], x0=x0, max_iterations=40)
    states = {}
    for name, (T, Cf) in (("initial", (T0, C0)), ("optimised", (res["T"], res["C"]))):
        T = np.array(T, dtype=np.float64); Cf = np.array(Cf, dtype=np.float64).reshape(-1, 3)
        ref = er.rows(T, Cf, g)
        ref.setflags(write=False)
        states[name] = (T, Cf, ref)
    yield prob, states
    prob.close()


def assert_rows(got, T, Cf, ref, piece_off, params):
    assert same(got["piece"], ref), differ(got["piece"], ref)[:8]
    cref = er.reduce_candidates(ref, T, piece_off)
    assert same(got["cand"], cref), differ(got["cand"], cref)[:8]
    assert np.array_equal(got["flags"], er.flags_of(cref, params)), (got["flags"], er.flags_of(cref, params))


@pytest.mark.parametrize("state", ["initial", "optimised"])
@pytest.mark.parametrize("layout", LAYOUTS, ids=lambda n: "P%d" % sum(n))
def test_bit_identical_to_the_restatement_at_the_wave_edges(frx, sc, pool, layout, state):
    _, states = pool
    T, Cf, ref = states[state]
    P = sum(layout)
    h = penalty_handle(frx, sc, layout)
    got = h.trajectory_extrema(T[:P], Cf[:6 * P])
    assert got["piece"].shape == (P, 10) and got["cand"].shape == (len(layout), 10) and got["flags"].dtype == np.uint32
    assert_rows(got, T[:P], Cf[:6 * P], ref[:P], h.piece_off, sc.ZHANGJIAJIE)
    assert np.array_equal(got["speed"], got["cand"][:, 0]) and np.array_equal(got["t_body_rate"], got["cand"][:, 9])
    h.close()


@pytest.mark.parametrize("state", ["initial", "optimised"])
def test_full_handle_host_function_forms_and_batch(frx, sc, pool, state):
    """The planning handle serves the call too; SPEED and ACC are frx_traj_max_rates' bits; blocking and _device forms, two calls, and a candidate alone or in
    a batch give the same bits."""
    prob, states = pool
    T, Cf, ref = states[state]
    a = prob.trajectory_extrema(T, Cf)
    assert_rows(a, T, Cf, ref, prob.piece_off, sc.ZHANGJIAJIE)
    Cp = Cf.reshape(-1, 6, 3)
    for i in range(len(T)):
        assert min(er.host_derivative_norms(Cp[i], T[i])) >= 2.220446049250313e-16, i    # the host's early-out is not in play: none left out
    mv, ma = frx.traj_max_rates(T, Cf)
    assert same(mv, a["piece"][:, 0]) and same(ma, a["piece"][:, 1])
    b = prob.trajectory_extrema(T, Cf)
    for k in ("piece", "cand", "flags"):
        assert np.array_equal(a[k], b[k], equal_nan=True)
    host = np.full(prob.P * 10, -7.0)
    Td, Cd, out = DevBuf(np.ascontiguousarray(T)), DevBuf(np.ascontiguousarray(Cf).reshape(-1)), DevBuf(host)
    prob.trajectory_extrema_device(Td.ptr.value, Cd.ptr.value, out.ptr.value, 0)
    assert same(out.get(host).reshape(-1, 10), a["piece"])
    for d in (Td, Cd, out):
        d.close()
    sl = slice(int(prob.piece_off[1]), int(prob.piece_off[2]))
    solo = penalty_handle(frx, sc, (sl.stop - sl.start,))
    r = solo.trajectory_extrema(T[sl], Cf[6 * sl.start:6 * sl.stop])
    assert same(r["piece"], a["piece"][sl]) and same(r["cand"][0], a["cand"][1]) and r["flags"][0] == a["flags"][1]
    solo.close()


def test_recorded_reference_maxima(frx, sc):
    """SPEED and ACC against Piece::getMaxVelRate / getMaxAccRate of the reference as recorded by tests/golden/make_extrema_golden.py, to the 1e-9 max(value, 1)
    tests/test_next_rows.py holds frx_traj_max_rates to; and against that function bit for bit."""
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", "refpin_extrema_max_rates.npz"))
    T, Cf = z["T"], z["C"].reshape(-1, 3)
    h = penalty_handle(frx, sc, (50,) * (len(T) // 50))                   # (a candidate's knot system holds about 128 pieces)
    got = h.trajectory_extrema(T, Cf)["piece"]
    h.close()
    assert (np.abs(got[:, 0] - z["max_vel"]) <= 1e-9 * np.maximum(z["max_vel"], 1.0)).all()
    assert (np.abs(got[:, 1] - z["max_acc"]) <= 1e-9 * np.maximum(z["max_acc"], 1.0)).all()
    mv, ma = frx.traj_max_rates(T, Cf)
    assert same(mv, got[:, 0]) and same(ma, got[:, 1])


@pytest.mark.parametrize("state", ["initial", "optimised"])
def test_dominates_the_sampling_check_on_the_same_handle(pool, state):
    """Every exact maximum >= the sampled one and the exact THRUST_MIN <= the sampled one, at M = kappa and M = 256, within the check's own 1e-12 (needed for
    BODY_RATE alone, where the check divides by a fast reciprocal root)."""
    prob, states = pool
    T, Cf, _ = states[state]
    ex = prob.trajectory_extrema(T, Cf)["piece"]
    for M in (prob.kappa, 256):
        ck = prob.trajectory_check(T, Cf, M)["piece"]
        for fe, fc in ((0, 1), (1, 5), (3, 3), (4, 4)):
            print(state, M, fe, float(np.min(ex[:, fe] - ck[:, fc])))
            assert (ex[:, fe] >= ck[:, fc] - TOL * np.maximum(1.0, np.abs(ck[:, fc]))).all(), (M, fe)
        assert (ex[:, 2] <= ck[:, 2] + TOL * np.maximum(1.0, np.abs(ck[:, 2]))).all(), M


def test_crafted_states(frx, sc, pool):
    """Each crafted state between two ordinary pieces (its neighbours' rows keep their bits) and as a candidate of its own (flags): values, times, flags; the
    device row is the restatement's bit for bit; (g) and (h) break a limit between the check's nodes at M = kappa, where the check sees nothing."""
    params = sc.ZHANGJIAJIE
    g = params["grav_acc"]
    _, states = pool
    T0, C0, ref0 = states["optimised"]
    Cp0 = C0.reshape(-1, 6, 3)
    crafted = es.crafted(params)
    names = list(crafted)
    T, Cp, piece_n = [], [], []
    for k, name in enumerate(names):                                     # candidates 0 .. n-1: (ordinary, crafted, ordinary)
        st = crafted[name]
        T += [T0[2 * k], st["T"], T0[2 * k + 1]]; Cp += [Cp0[2 * k], st["c"], Cp0[2 * k + 1]]; piece_n.append(3)
    for name in names:                                                   # candidates n .. 2n-1: the crafted piece alone
        T.append(crafted[name]["T"]); Cp.append(crafted[name]["c"]); piece_n.append(1)
    T = np.array(T); Cf = np.array(Cp).reshape(-1, 3)
    h = penalty_handle(frx, sc, piece_n)
    got = h.trajectory_extrema(T, Cf)
    ref = er.rows(T, Cf, g)
    assert_rows(got, T, Cf, ref, h.piece_off, params)
    check = h.trajectory_check(T, Cf, KAPPA)
    n = len(names)
    for k, name in enumerate(names):
        st = crafted[name]
        row = got["piece"][3 * k + 1]
        bad = er.bound_failures(row, st["c"], st["T"], g) + er.expectation_failures(row, st["expect"])
        assert not bad, (name, bad)
        assert same(got["piece"][3 * k], ref0[2 * k]) and same(got["piece"][3 * k + 2], ref0[2 * k + 1]), name
        assert same(got["piece"][3 * n + k], row), name
        fl = int(got["flags"][n + k])
        assert fl & st["set"] == st["set"] and fl & st["clear"] == 0, (name, fl)
    f = got["piece"][3 * names.index("f_two_equal_maxima") + 1]
    assert abs(f[5] - 0.25) < 1e-6 or abs(f[5] - 0.75) < 1e-6
    kg, kh = n + names.index("g_speed_between_nodes"), n + names.index("h_thrust_between_nodes")
    assert not check["flags"][kg] & frx.CHECK_FLAG_SPEED and got["flags"][kg] & frx.CHECK_FLAG_SPEED
    assert not check["flags"][kh] & frx.CHECK_FLAG_THRUST_MIN and got["flags"][kh] & frx.CHECK_FLAG_THRUST_MIN
    ki = n + names.index("i_free_fall")
    assert got["cand"][ki, 2] == 0.0 and got["cand"][ki, 3] == 0.0 and np.isnan(got["cand"][ki, 4]) and got["flags"][ki] & frx.CHECK_FLAG_NONFINITE
    h.close()


def test_bad_pieces_poison_their_own_rows_only(frx, sc, pool):
    """(j) a NaN coefficient, T = inf, T = 0 and T < 0 in four pieces of one candidate: those rows are all NaN, the candidate is NONFINITE, every other row and
    candidate has the bits it has without them"""
    _, states = pool
    T0, C0, ref0 = states["optimised"]
    piece_n = (4, 5, 3)
    P = sum(piece_n)
    T = np.array(T0[:P]); Cp = np.array(C0[:6 * P]).reshape(-1, 6, 3)
    h = penalty_handle(frx, sc, piece_n)
    clean = h.trajectory_extrema(T, Cp.reshape(-1, 3))
    where = (4, 5, 7, 8)                                                 # all in candidate 1
    for q, (t, c) in zip(where, es.bad_pieces(np.random.default_rng(3))):
        T[q] = t; Cp[q] = c
    got = h.trajectory_extrema(T, Cp.reshape(-1, 3))
    h.close()
    assert np.isnan(got["piece"][list(where)]).all()
    others = np.setdiff1d(np.arange(P), where)
    assert same(got["piece"][others], clean["piece"][others]) and same(got["piece"][others], ref0[others])
    assert got["flags"][1] == frx.CHECK_FLAG_NONFINITE and np.isnan(got["cand"][1, :5]).all()
    for b in (0, 2):
        assert same(got["cand"][b], clean["cand"][b]) and got["flags"][b] == clean["flags"][b]


def test_abi_and_argument_errors(frx, sc, pool):
    prob, states = pool
    T, Cf, _ = states["initial"]
    L = frx.lib()
    for name in ("frx_trajectory_extrema", "frx_trajectory_extrema_device"):
        assert name in frx.ABI_SYMBOLS and hasattr(L, name)
    cand = np.zeros((prob.B, 10))
    Tc, Cc = np.ascontiguousarray(T), np.ascontiguousarray(Cf).reshape(-1)
    assert L.frx_trajectory_extrema(None, Tc.ctypes.data, Cc.ctypes.data, None, cand.ctypes.data, None) == -1
    assert L.frx_trajectory_extrema(prob.h, None, Cc.ctypes.data, None, cand.ctypes.data, None) == -1
    assert L.frx_trajectory_extrema(prob.h, Tc.ctypes.data, None, None, cand.ctypes.data, None) == -1
    assert L.frx_trajectory_extrema(prob.h, Tc.ctypes.data, Cc.ctypes.data, None, None, None) == -1
    assert L.frx_trajectory_extrema_device(prob.h, 8, 8, None, None) == -1
    assert L.frx_trajectory_extrema(prob.h, Tc.ctypes.data, Cc.ctypes.data, None, cand.ctypes.data, None) == 0      # piece_out and flags may be NULL
    assert same(cand, prob.trajectory_extrema(T, Cf)["cand"])
    with pytest.raises(ValueError):
        prob.trajectory_extrema(T[:-1], Cf)
    with pytest.raises(ValueError):
        prob.trajectory_extrema(T, Cf[:-6])
