"""frx_trajectory_gates on the device: bit for bit against the float64 restatement (tests/gates_reference.py) at the wave's edges, between the forms, calls,
batches and kinds of handle, on the crafted states of tests/gate_states.py, and against frx_trajectory_sample at the reported times.

A handle holds candidates of up to 128 pieces (frx_problem_create refuses a larger knot system with FRX_ERR_CAPACITY), so the longest candidate here has 128
pieces - two full strides of the kernel's walk - and state (k) has its only crossing in piece 127; the 130-piece form of (k) is held to its closed form on
the restatement in tests/test_trajectory_gates_cpu.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gate_states as gs  # noqa: E402
import gates_reference as gr  # noqa: E402

pytestmark = pytest.mark.gpu

KAPPA = 16
LONG = 128                                                              # the most pieces a candidate of a handle can have
BOX = np.concatenate([np.vstack([np.eye(3), np.diag([2.0, 2.0, 4.0])]), np.vstack([-np.eye(3), np.diag([-2.0, -2.0, 0.0])])], axis=1)
# pieces per candidate and gates per candidate: 1, 63, 64, 65 and LONG pieces, 0, 1 and 3 gates, a candidate without gates first, in the middle and last
CASES = [((1,), (1,)), ((1,), (3,)), ((63, 64), (0, 3)), ((63, 64), (1, 0)), ((65, 1, LONG), (3, 0, 1)), ((65, 1, LONG), (0, 1, 3))]
EPS = np.finfo(np.float64).eps


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def differ(a, b):
    """where two arrays differ as uint64; two values that are both not a number count as equal"""
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


def params_of(sc):
    p = sc.ZHANGJIAJIE
    return (p["horiz_half_len"], p["horiz_half_len"], p["vert_half_len"]), p["grav_acc"]


def penalty_handle(frx, sc, piece_n):
    P = int(np.sum(piece_n))
    return frx.PenaltyProblem(sc.ZHANGJIAJIE, list(piece_n), [0] * P, [BOX], qd_intervals=KAPPA)


def offsets(counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)


@pytest.fixture(scope="module")
def pool(frx, sc):
    """130 pieces of two candidates (the pool of the extrema test) at the initial guess and after a short optimisation, with the candidates' own gates and the
    restatement's rows for them: computed once, shared, left unchanged"""
    ell, g = params_of(sc)
    cands = sc.make_batch(0, 2, 65, 16)
    prob = frx.Problem(cands, sc.ZHANGJIAJIE, qd_intervals=KAPPA)
    x0 = prob.initial_guess()
    T0, C0 = prob.forward(x0)
    res = prob.optimize(sc.ZHANGJIAJIE["opt_rel_tol"], x0=x0, max_iterations=40)
    gates = np.concatenate([gs.candidate_gates(c) for c in cands])
    gate_off = offsets([len(c.gates) for c in cands])
    states = {}
    for name, (T, Cf) in (("initial", (T0, C0)), ("optimised", (res["T"], res["C"]))):
        T = np.array(T, dtype=np.float64); Cf = np.array(Cf, dtype=np.float64).reshape(-1, 3)
        ref = gr.rows(T, Cf, prob.piece_off, gates, gate_off, ell, g)
        for a in (T, Cf, ref):
            a.setflags(write=False)
        states[name] = (T, Cf, ref)
    yield prob, states, gates, gate_off
    prob.close()


def tiled(T, Cf, P):
    """the first P pieces of the pool, the pool repeated where P exceeds it"""
    idx = np.arange(P) % len(T)
    return np.ascontiguousarray(T[idx]), np.ascontiguousarray(Cf.reshape(-1, 6, 3)[idx]).reshape(-1, 3)


def gates_through(rng, T, Cf, piece_off, counts):
    """counts[b] gates for candidate b, each through a random point of a random piece of that candidate"""
    Cp = Cf.reshape(-1, 6, 3)
    out = []
    for b, n in enumerate(counts):
        for _ in range(n):
            k = int(rng.integers(piece_off[b], piece_off[b + 1]))
            out.append(gs.random_gates(rng, float(T[k]), Cp[k], 1, inner=0.1)[0])
    return np.array(out).reshape(-1, 9), offsets(counts)


def assert_rows(got, ref, gate_off):
    assert same(got["gate"], ref), (differ(got["gate"], ref)[:8], got["gate"], ref)
    assert np.array_equal(got["flags"], gr.flags_of(ref, gate_off)), (got["flags"], gr.flags_of(ref, gate_off))


@pytest.mark.parametrize("state", ["initial", "optimised"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "pieces%s-gates%s" % ("_".join(map(str, c[0])), "_".join(map(str, c[1]))))
def test_bit_identical_to_the_restatement_at_the_wave_edges(frx, sc, pool, case, state):
    ell, g = params_of(sc)
    _, states, _, _ = pool
    piece_n, gate_n = case
    T, Cf = tiled(states[state][0], states[state][1], sum(piece_n))
    h = penalty_handle(frx, sc, piece_n)
    gates, gate_off = gates_through(np.random.default_rng(17 + sum(gate_n)), T, Cf, h.piece_off, gate_n)
    got = h.trajectory_gates(T, Cf, gates, gate_off)
    h.close()
    ref = gr.rows(T, Cf, offsets(piece_n), gates, gate_off, ell, g)
    assert got["gate"].shape == (sum(gate_n), 10) and got["flags"].shape == (len(piece_n),) and got["flags"].dtype == np.uint32
    assert_rows(got, ref, gate_off)
    assert (ref[:, gr.N_CROSS] >= 1).all()                                # every gate was laid through its candidate
    assert np.array_equal(got["margin"], got["gate"][:, 2]) and np.array_equal(got["normal_speed"], got["gate"][:, 9])


@pytest.mark.parametrize("state", ["initial", "optimised"])
def test_forms_calls_batches_and_handles_give_the_same_bits(frx, sc, pool, state):
    """The planning handle with the candidates' own gates: the restatement's bits; two calls, the blocking and the _device form, a candidate alone or in the
    batch, and a penalty handle of the same layout all give the same bits."""
    prob, states, gates, gate_off = pool
    T, Cf, ref = states[state]
    a = prob.trajectory_gates(T, Cf, gates, gate_off)
    assert_rows(a, ref, gate_off)
    b = prob.trajectory_gates(T, Cf, gates, gate_off)
    assert same(a["gate"], b["gate"]) and np.array_equal(a["flags"], b["flags"])
    host = np.full(len(gates) * 10, -7.0)
    bufs = [DevBuf(np.ascontiguousarray(T)), DevBuf(np.ascontiguousarray(Cf).reshape(-1)), DevBuf(gate_off), DevBuf(np.ascontiguousarray(gates).reshape(-1)), DevBuf(host)]
    prob.trajectory_gates_device(bufs[0].ptr.value, bufs[1].ptr.value, len(gates), bufs[2].ptr.value, bufs[3].ptr.value, bufs[4].ptr.value, 0)
    dev = bufs[4].get(host).reshape(-1, 10)
    for d in bufs:
        d.close()
    assert same(dev, a["gate"])
    assert np.array_equal(frx.gate_flags(dev, gate_off), a["flags"])
    pen = penalty_handle(frx, sc, np.diff(prob.piece_off))
    c = pen.trajectory_gates(T, Cf, gates, gate_off)
    pen.close()
    assert same(c["gate"], a["gate"]) and np.array_equal(c["flags"], a["flags"])
    sl = slice(int(prob.piece_off[1]), int(prob.piece_off[2])); gl = slice(int(gate_off[1]), int(gate_off[2]))
    solo = penalty_handle(frx, sc, (sl.stop - sl.start,))
    r = solo.trajectory_gates(T[sl], Cf[6 * sl.start:6 * sl.stop], gates[gl], [0, gl.stop - gl.start])
    solo.close()
    assert same(r["gate"], a["gate"][gl]) and r["flags"][0] == a["flags"][1]


def test_crafted_states_between_ordinary_candidates(frx, sc, pool):
    """(ordinary, crafted, ordinary, crafted, ..., ordinary): every row is the restatement's bit for bit; the ordinary candidates' rows are the bits they have in a
    batch without the crafted ones (so state (i) poisons its own rows only); the crafted rows hold their closed forms and flags."""
    params = sc.ZHANGJIAJIE
    ell, g = params_of(sc)
    _, states, _, _ = pool
    T0, C0, _ = states["optimised"]
    Cp0 = C0.reshape(-1, 6, 3)
    crafted = gs.crafted(params, long_n=LONG)
    names = list(crafted)
    rng = np.random.default_rng(23)
    ordinary = []
    for j in range(len(names) + 1):                                      # four pieces of the pool each, one gate through the second
        sl = slice(4 * j, 4 * j + 4)
        ordinary.append((T0[sl], Cp0[sl], gs.random_gates(rng, float(T0[4 * j + 1]), Cp0[4 * j + 1], 1, inner=0.1)))
    seq = [ordinary[0]]
    for j, name in enumerate(names):
        st = crafted[name]
        seq += [(st["T"], st["C"], st["gates"]), ordinary[j + 1]]

    def run(cands):
        piece_n, gate_n = [len(t) for t, _, _ in cands], [len(gt) for _, _, gt in cands]
        T = np.concatenate([t for t, _, _ in cands]); Cf = np.concatenate([c for _, c, _ in cands]).reshape(-1, 3)
        gates, gate_off = np.concatenate([gt for _, _, gt in cands]), offsets(gate_n)
        h = penalty_handle(frx, sc, piece_n)
        got = h.trajectory_gates(T, Cf, gates, gate_off)
        h.close()
        return got, gr.rows(T, Cf, offsets(piece_n), gates, gate_off, ell, g), gate_off

    got, ref, gate_off = run(seq)
    assert_rows(got, ref, gate_off)
    alone, ref_alone, off_alone = run(ordinary)
    assert_rows(alone, ref_alone, off_alone)
    for j in range(len(ordinary)):
        assert same(got["gate"][gate_off[2 * j]], alone["gate"][j]) and got["flags"][2 * j] == alone["flags"][j], j
    for j, name in enumerate(names):
        st, b = crafted[name], 2 * j + 1
        rows = got["gate"][gate_off[b]:gate_off[b + 1]]
        for r, e in zip(rows, st["expect"]):
            if isinstance(e, str):
                assert np.isnan(r).all(), (name, r)
            else:
                assert not gr.expectation_failures(r, e), (name, gr.expectation_failures(r, e), r)
        fl = int(got["flags"][b])
        assert fl & st["set"] == st["set"] and fl & st["clear"] == 0, (name, fl)
    i = names.index("i_nan_gate")                                        # the good gate beside the bad one, and the candidate's flag
    assert not np.isnan(got["gate"][gate_off[2 * i + 1] + 1]).any() and got["flags"][2 * i + 1] & frx.GATE_FLAG_NONFINITE


def rotation(q):
    """R = [xB yB zB] of a quaternion (w, x, y, z), Hamilton convention"""
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


@pytest.mark.parametrize("state", ["initial", "optimised"])
def test_reported_crossings_against_trajectory_sample(frx, sc, pool, state):
    """Every reported TIME sampled with frx_trajectory_sample: |n.(pos - c)| <= 256 eps S there (S = |c| + sum_k |c_k| T^k of the reported piece), and U, V,
    NORMAL_SPEED from the sample's pos / vel, REACH_U / V from its quaternion, to 1e-9 max(1, |value|)."""
    ell, _ = params_of(sc)
    E = np.array(ell)
    prob, states, gates, gate_off = pool
    T, Cf, _ = states[state]
    Cp = Cf.reshape(-1, 6, 3)
    got = prob.trajectory_gates(T, Cf, gates, gate_off)["gate"]
    S = int(np.diff(gate_off).max())
    times = np.zeros((prob.B, S))
    for b in range(prob.B):
        t = got[gate_off[b]:gate_off[b + 1], gr.TIME]
        times[b, :len(t)] = t
    smp = prob.trajectory_sample(T, Cf, S, times=times)
    checked = 0
    for b in range(prob.B):
        for i, gi in enumerate(range(gate_off[b], gate_off[b + 1])):
            r = got[gi]
            if not r[gr.N_CROSS] > 0:
                continue
            c, a, bb = gates[gi, 0:3], gates[gi, 3:6], gates[gi, 6:9]
            eu, ev, n = a / np.linalg.norm(a), bb / np.linalg.norm(bb), np.cross(a, bb) / np.linalg.norm(np.cross(a, bb))
            k = int(prob.piece_off[b]) + int(r[gr.PIECE])
            size = gr.scale(Cp[k], T[k], gates[gi])
            pos, vel, R = smp["pos"][b, i], smp["vel"][b, i], rotation(smp["quat"][b, i])
            d = pos - c
            print(state, b, i, float(n @ d) / (EPS * size))
            assert abs(n @ d) <= 256 * EPS * size, (b, i, n @ d, size)
            want = {gr.U: eu @ d, gr.V: ev @ d, gr.NORMAL_SPEED: n @ vel, gr.REACH_U: np.linalg.norm(E * (R.T @ eu)), gr.REACH_V: np.linalg.norm(E * (R.T @ ev))}
            want[gr.MARGIN] = min(np.linalg.norm(a) - abs(want[gr.U]) - want[gr.REACH_U], np.linalg.norm(bb) - abs(want[gr.V]) - want[gr.REACH_V])
            for f, v in want.items():
                assert abs(r[f] - v) <= 1e-9 * max(1.0, abs(v)), (b, i, gr.FIELDS[f], r[f], v)
            checked += 1
    assert checked >= len(gates) // 2                                    # most of the candidates' own gates are crossed


def test_abi_and_argument_errors(frx, sc, pool):
    prob, states, gates, gate_off = pool
    T, Cf, _ = states["initial"]
    L = frx.lib()
    for name in ("frx_gate_from_corners", "frx_trajectory_gates", "frx_trajectory_gates_device", "frx_gate_flags"):
        assert name in frx.ABI_SYMBOLS and hasattr(L, name)
    Tc, Cc, gc = np.ascontiguousarray(T), np.ascontiguousarray(Cf).reshape(-1), np.ascontiguousarray(gates).reshape(-1)
    off = np.ascontiguousarray(gate_off, dtype=np.int32)
    rows = np.zeros((len(gates), 10))
    good = [prob.h, Tc.ctypes.data, Cc.ctypes.data, off.ctypes.data, gc.ctypes.data, rows.ctypes.data, None]
    for k in range(6):
        args = list(good)
        args[k] = None
        assert L.frx_trajectory_gates(*args) == -1, k
    for bad in ([1, 16, 32], [0, 17, 16], [0, 0, 0], [0, -1, 3]):         # gate_off[0] != 0, falling, no gates at all, falling below 0
        o = np.array(bad, np.int32)
        assert L.frx_trajectory_gates(prob.h, Tc.ctypes.data, Cc.ctypes.data, o.ctypes.data, gc.ctypes.data, rows.ctypes.data, None) == -1, bad
    assert L.frx_trajectory_gates(*good) == 0                            # flags may be NULL
    assert same(rows, prob.trajectory_gates(T, Cf, gates, gate_off)["gate"])
    for k in (0, 1, 2, 4, 5, 6):
        args = [prob.h, 8, 8, 1, 8, 8, 8, None]
        args[k] = None
        assert L.frx_trajectory_gates_device(*args) == -1, k
    assert L.frx_trajectory_gates_device(prob.h, 8, 8, 0, 8, 8, 8, None) == -1
    assert L.frx_trajectory_gates_device(prob.h, 8, 8, -3, 8, 8, 8, None) == -1
    with pytest.raises(ValueError):
        prob.trajectory_gates(T[:-1], Cf, gates, gate_off)
    with pytest.raises(ValueError):
        prob.trajectory_gates(T, Cf, gates[:-1], gate_off)
    with pytest.raises(ValueError):
        prob.trajectory_gates(T, Cf, gates, gate_off[:-1])
