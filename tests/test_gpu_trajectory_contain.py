"""frx_trajectory_contain on the device: bit for bit against the float64 restatement (tests/contain_reference.py) for ragged batches at every group width
(Kmax 8, 14 and 70: G = 8, 16 and 64 with a stride loop), between the forms, calls, batches and kinds of handle, on the crafted states of
tests/contain_states.py, and against frx_trajectory_check at M = 256."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import contain_reference as cn  # noqa: E402
import contain_states as cs  # noqa: E402

pytestmark = pytest.mark.gpu

KAPPA = 16
CASES = [(1,), (7,), (8, 9), (65, 1, 7)]                                 # pieces per candidate: 1, 7, 8, 9 and 65 pieces, ragged batches
# The pool's trajectories keep well inside their cells (CENTRE about -0.9): at slack 0 and safe_margin most faces are skipped or never touched.  Pulled in by
# 0.5 and 1.0 the faces cut through the paths, and the degree-16 task has contacts to find on ordinary data.
SLACKS_RAGGED = (0.0, 1.0)
SLACKS_FORMS = (0.08, 0.5)


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


def offsets(counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)


def penalty_handle(frx, sc, piece_n, polys):
    """a penalty handle whose piece i lives in polys[i]"""
    P = int(np.sum(piece_n))
    assert len(polys) == P
    return frx.PenaltyProblem(sc.ZHANGJIAJIE, list(piece_n), list(range(P)), list(polys), qd_intervals=KAPPA)


def padded(hp, K):
    """the polytope hp with faces added up to K: copies of its own faces moved outwards by 0.02, 0.04, ... (near enough to be touched, never the first to be)"""
    cols = [hp[:, k] for k in range(hp.shape[1])]
    j = 0
    while len(cols) < K:
        src = hp[:, j % hp.shape[1]]
        n = src[:3] / np.linalg.norm(src[:3])
        cols.append(np.concatenate([src[:3], src[3:] + 0.02 * (1 + j // hp.shape[1]) * n]))
        j += 1
    return np.array(cols).T.copy()


@pytest.fixture(scope="module")
def pool(frx, sc):
    """130 pieces of two candidates at the initial guess and after about 30 iterations, with their corridor cells and the restatement's rows at the slacks of
    the tests: computed once, shared, left unchanged"""
    params = sc.ZHANGJIAJIE
    cands = sc.make_batch(0, 2, 65, 16)
    prob = frx.Problem(cands, params, qd_intervals=KAPPA)
    assert prob.P == prob.Pc and prob.Kmax == 8                          # one fine piece per corridor cell, in candidate order
    polys = [h for c in cands for h in c.h_polys]
    x0 = prob.initial_guess()
    T0, C0 = prob.forward(x0)
    res = prob.optimize(params["opt_rel_tol"], x0=x0, max_iterations=30)
    states = {}
    for name, (T, Cf) in (("initial", (T0, C0)), ("optimised", (res["T"], res["C"]))):
        T = np.array(T, dtype=np.float64); Cf = np.array(Cf, dtype=np.float64).reshape(-1, 3)
        ref = {s: cn.rows(T, Cf, prob.piece_off, polys, params, s) for s in SLACKS_RAGGED + SLACKS_FORMS}
        for a in (T, Cf) + tuple(ref.values()):
            a.setflags(write=False)
        states[name] = (T, Cf, ref)
    yield prob, cands, polys, states
    prob.close()


def tiled(T, Cf, polys, P):
    """the first P pieces of the pool with their cells"""
    assert P <= len(T)
    return np.ascontiguousarray(T[:P]), np.ascontiguousarray(Cf.reshape(-1, 6, 3)[:P]).reshape(-1, 3), polys[:P]


def assert_rows(got, ref, T, piece_off):
    assert same(got["piece"], ref), (differ(got["piece"], ref)[:8], got["piece"][differ(got["piece"], ref)[:4, 0]], ref[differ(got["piece"], ref)[:4, 0]])
    cref = cn.reduce_candidates(ref, T, piece_off)
    assert same(got["cand"], cref), (got["cand"], cref)
    assert np.array_equal(got["flags"], cn.flags_of(cref, piece_off)), (got["flags"], cn.flags_of(cref, piece_off))


@pytest.mark.parametrize("state", ["initial", "optimised"])
@pytest.mark.parametrize("K", [8, 14, 70])
def test_bit_identical_to_the_restatement_for_ragged_batches(frx, sc, pool, K, state):
    """Kmax 8, 14 and 70 (G = 8, 16, 64; 70 faces take a second stride) x batches of 1, 7, 8 + 9 and 65 + 1 + 7 pieces, at slack 0 and 1"""
    params = sc.ZHANGJIAJIE
    _, _, polys, states = pool
    contacts = 0
    for piece_n in CASES:
        T, Cf, hp = tiled(states[state][0], states[state][1], polys, sum(piece_n))
        hp = [padded(h, K) if i % (1 + K // 10) == 0 else h for i, h in enumerate(hp)]    # (pieces of fewer faces than Kmax beside the full ones)
        h = penalty_handle(frx, sc, piece_n, hp)
        assert h.Kmax == K and np.array_equal(h.piece_off, offsets(piece_n))
        for slack in SLACKS_RAGGED:
            got = h.trajectory_contain(T, Cf, slack)
            ref = states[state][2][slack][:len(T)] if K == 8 and len(piece_n) == 1 else cn.rows(T, Cf, offsets(piece_n), hp, params, slack)
            assert got["piece"].shape == (len(T), 8) and got["cand"].shape == (len(piece_n), 8) and got["flags"].dtype == np.uint32
            assert_rows(got, ref, T, offsets(piece_n))
            assert np.array_equal(got["outside"], got["cand"][:, 1]) and np.array_equal(got["k_centre"], got["cand"][:, 7])
            contacts += int(ref[:, cn.N_CONTACT].sum())
        h.close()
    print(K, state, "contacts", contacts)
    assert contacts > 0                                                  # the degree-16 task had contacts to find


@pytest.mark.parametrize("state", ["initial", "optimised"])
def test_forms_calls_batches_and_handles_give_the_same_bits(frx, sc, pool, state):
    """The planning handle: the restatement's bits; two calls, the blocking and the _device form (with frx_contain_fold), a candidate alone or in the batch, and
    a penalty handle of the same layout all give the same bits."""
    params = sc.ZHANGJIAJIE
    prob, cands, polys, states = pool
    T, Cf, ref = states[state]
    assert SLACKS_FORMS[0] == params["safe_margin"]                      # the face the penalty aims at
    for slack in SLACKS_FORMS:
        a = prob.trajectory_contain(T, Cf, slack)
        assert_rows(a, ref[slack], T, prob.piece_off)
        b = prob.trajectory_contain(T, Cf, slack)
        assert same(a["piece"], b["piece"]) and same(a["cand"], b["cand"]) and np.array_equal(a["flags"], b["flags"])
        host = np.full(prob.P * 8, -7.0)
        bufs = [DevBuf(np.ascontiguousarray(T)), DevBuf(np.ascontiguousarray(Cf).reshape(-1)), DevBuf(host)]
        prob.trajectory_contain_device(bufs[0].ptr.value, bufs[1].ptr.value, bufs[2].ptr.value, slack, 0)
        dev = bufs[2].get(host).reshape(-1, 8)
        for d in bufs:
            d.close()
        assert same(dev, a["piece"])
        cand, flags = frx.contain_fold(dev, T, prob.piece_off)
        assert same(cand, a["cand"]) and np.array_equal(flags, a["flags"])
        pen = penalty_handle(frx, sc, np.diff(prob.piece_off), polys)
        c = pen.trajectory_contain(T, Cf, slack)
        pen.close()
        assert same(c["piece"], a["piece"]) and same(c["cand"], a["cand"]) and np.array_equal(c["flags"], a["flags"])
        sl = slice(int(prob.piece_off[1]), int(prob.piece_off[2]))
        solo = frx.Problem([cands[1]], params, qd_intervals=KAPPA)
        r = solo.trajectory_contain(T[sl], Cf[6 * sl.start:6 * sl.stop], slack)
        solo.close()
        assert same(r["piece"], a["piece"][sl]) and same(r["cand"][0], a["cand"][1]) and r["flags"][0] == a["flags"][1]


def _run_states(frx, sc, group, ordinary):
    """(ordinary, crafted, ordinary, crafted, ..., ordinary) on one penalty handle: (got, piece offsets, T, Cf, polys)"""
    seq = [ordinary[0]]
    for j, st in enumerate(group):
        seq += [(st["T"], st["C"], st["polys"]), ordinary[j + 1]]
    piece_n = [len(t) for t, _, _ in seq]
    T = np.concatenate([t for t, _, _ in seq]); Cf = np.concatenate([np.asarray(c).reshape(-1, 3) for _, c, _ in seq])
    hp = [h for _, _, hs in seq for h in hs]
    return piece_n, T, Cf, hp


def test_crafted_states_between_ordinary_candidates(frx, sc, pool):
    """Every crafted state between ordinary candidates, the states of one slack in one batch: every row is the restatement's bit for bit, the ordinary candidates'
    rows are the bits they have without the crafted ones (state (k) poisons its own candidate only), the crafted rows hold their closed forms and flags.  At
    slack 0 the batch is also held to frx_trajectory_check at M = 256 - and state (h) to M = 2, which sees nothing."""
    params = sc.ZHANGJIAJIE
    _, _, polys, states = pool
    T0, C0, _ = states["optimised"]
    Cp0 = C0.reshape(-1, 6, 3)
    crafted = cs.crafted(params)
    for slack in sorted({st["slack"] for st in crafted.values()}):
        names = [n for n, st in crafted.items() if st["slack"] == slack]
        ordinary = [(T0[4 * j:4 * j + 4], Cp0[4 * j:4 * j + 4], polys[4 * j:4 * j + 4]) for j in range(len(names) + 1)]
        piece_n, T, Cf, hp = _run_states(frx, sc, [crafted[n] for n in names], ordinary)
        h = penalty_handle(frx, sc, piece_n, hp)
        got = h.trajectory_contain(T, Cf, slack)
        chk = h.trajectory_check(T, Cf, 256)
        chk2 = h.trajectory_check(T, Cf, 2)
        h.close()
        off = offsets(piece_n)
        assert_rows(got, cn.rows(T, Cf, off, hp, params, slack), T, off)
        for j in range(len(ordinary)):                                    # every ordinary candidate alone on its own handle
            To, Co, hpo = ordinary[j][0], ordinary[j][1].reshape(-1, 3), ordinary[j][2]
            ho = penalty_handle(frx, sc, [len(To)], hpo)
            alone = ho.trajectory_contain(To, Co, slack)
            ho.close()
            sl = slice(off[2 * j], off[2 * j + 1])
            assert same(got["piece"][sl], alone["piece"]) and same(got["cand"][2 * j], alone["cand"][0]) and got["flags"][2 * j] == alone["flags"][0], j
        for j, name in enumerate(names):
            st, b = crafted[name], 2 * j + 1
            rows = got["piece"][off[b]:off[b + 1]]
            for r, e in zip(rows, st["expect"]):
                if isinstance(e, str):
                    assert np.isnan(r).all(), (name, r)
                else:
                    assert not cn.expectation_failures(r, e), (name, cn.expectation_failures(r, e), r)
            if st["cand"] is not None:
                assert not cn.expectation_failures(got["cand"][b], st["cand"]), (name, cn.expectation_failures(got["cand"][b], st["cand"]), got["cand"][b])
            fl = int(got["flags"][b])
            assert fl & st["set"] == st["set"] and fl & st["clear"] == 0, (name, fl)
        if slack == 0.0:
            assert_consistent_with_the_check(got, chk)
            b = 2 * names.index("h_between_the_nodes") + 1
            assert chk2["corridor"][b] < 0.0 and not chk2["flags"][b] & frx.CHECK_FLAG_CORRIDOR and got["n_contact"][b] == 4 and got["flags"][b] & frx.CHECK_FLAG_CORRIDOR


def assert_consistent_with_the_check(got, chk):
    """wherever the certificate says inside (OUTSIDE == 0), the check's CORRIDOR <= 0; wherever the check has CORRIDOR > 0, the certificate is flagged.  (A piece
    in free fall has no attitude: the check's CORRIDOR is not a number there and says neither.)"""
    pc, cc = chk["piece"][:, 0], chk["candidate"][:, 0]
    with np.errstate(invalid="ignore"):
        inside = (got["piece"][:, cn.OUTSIDE] == 0.0) & ~np.isnan(pc)
        assert (pc[inside] <= 0.0).all(), (np.argwhere(inside & (pc > 0.0))[:5], pc[inside].max())
        assert (got["piece"][pc > 0.0, cn.OUTSIDE] > 0.0).all()
        cin = (got["cand"][:, cn.OUTSIDE] == 0.0) & ~np.isnan(cc)
        assert (cc[cin] <= 0.0).all()
        assert (got["flags"][cc > 0.0] & 1 == 1).all()
    print("pieces inside", int(inside.sum()), "of", len(pc), "check says outside", int((pc > 0.0).sum()))


@pytest.mark.parametrize("state", ["initial", "optimised"])
def test_consistent_with_the_dense_check_at_slack_zero(frx, sc, pool, state):
    prob, _, _, states = pool
    T, Cf, _ = states[state]
    got = prob.trajectory_contain(T, Cf, 0.0)
    chk = prob.trajectory_check(T, Cf, 256)
    assert_consistent_with_the_check(got, chk)
    # the enclosure: CENTRE + min(eh, ev) <= max sd <= CENTRE + max(eh, ev), and the check's samples cannot exceed max sd
    ell = (sc.ZHANGJIAJIE["horiz_half_len"], sc.ZHANGJIAJIE["vert_half_len"])
    assert (chk["piece"][:, 0] <= got["piece"][:, cn.CENTRE] + max(ell) + 1e-12).all()


def test_abi_and_argument_errors(frx, sc, pool):
    prob, _, _, states = pool
    T, Cf, _ = states["initial"]
    L = frx.lib()
    Tc, Cc = np.ascontiguousarray(T), np.ascontiguousarray(Cf).reshape(-1)
    piece = np.zeros((prob.P, 8)); cand = np.zeros((prob.B, 8))
    good = [prob.h, Tc.ctypes.data, Cc.ctypes.data, 0.0, piece.ctypes.data, cand.ctypes.data, None]
    for k in (0, 1, 2, 5):
        args = list(good)
        args[k] = None
        assert L.frx_trajectory_contain(*args) == -1, k
    for bad in (np.nan, np.inf):
        args = list(good)
        args[3] = bad
        assert L.frx_trajectory_contain(*args) == -1
        assert L.frx_trajectory_contain_device(prob.h, 8, 8, bad, 8, None) == -1
    assert L.frx_trajectory_contain(*good) == 0                          # flags may be NULL
    ref = prob.trajectory_contain(T, Cf, 0.0)
    assert same(piece, ref["piece"]) and same(cand, ref["cand"])
    good[4] = None                                                       # and so may piece_out
    cand[:] = 0.0
    assert L.frx_trajectory_contain(*good) == 0 and same(cand, ref["cand"])
    with pytest.raises(ValueError):
        prob.trajectory_contain(T[:-1], Cf)
