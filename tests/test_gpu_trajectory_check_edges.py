"""frx_trajectory_check at the edges of its launch geometry and of its tie rules (tests/check_states.py): every lanes-per-piece class from M and
from the LDS rule, partial and empty waves, neighbours of different K inside a wave, the capacity edge, exact ties, NaN order, and every flag
on both sides of its comparison.  Values against tests/check_reference.py to the TOL of test_gpu_trajectory_check; whatever is stated as
exact (ties, indices, worst_t, flags, NaN placement) with ==."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import check_states as cs  # noqa: E402
from test_gpu_trajectory_check import DevBuf, assert_agrees  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = -7.0
PAD = 4 * 32 * 8                                                       # sentinel doubles behind the device rows: a whole workgroup's rows at ppw = 32
FRX_ERR_CAPACITY = -5


def handle(frx, sc, st):
    return frx.PenaltyProblem(st.params(sc.ZHANGJIAJIE), st.counts, st.piece_poly, st.polys, qd_intervals=8)


def same(a, b):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in ("piece", "candidate", "flags"))


def device_rows(prob, st, M):
    """The piece rows of the device form, written into a buffer pre-filled with a sentinel; nothing is written behind row P - 1 (a last wave
    that took itself for full would write the rows of pieces that do not exist)."""
    host = np.full(st.P * 8 + PAD, SENTINEL)
    Td, Cd, out = DevBuf(np.ascontiguousarray(st.T)), DevBuf(np.ascontiguousarray(st.Cf).reshape(-1)), DevBuf(host)
    try:
        prob.trajectory_check_device(Td.ptr.value, Cd.ptr.value, out.ptr.value, M, 0)
        got = out.get(host)
        assert (got[st.P * 8:] == SENTINEL).all()
        return got[:st.P * 8].reshape(-1, 8)
    finally:
        for d in (Td, Cd, out):
            d.close()


def solo_row(frx, sc, st, q, M):
    """Piece q of the state alone in a handle of its own."""
    solo = frx.PenaltyProblem(st.params(sc.ZHANGJIAJIE), [1], [0], [st.piece_polys[q]], qd_intervals=8)
    try:
        return solo.trajectory_check(st.T[q:q + 1], st.Cf[6 * q:6 * q + 6], M)["piece"][0]
    finally:
        solo.close()


def check_geometry_state(frx, sc, st, solo_pieces=()):
    """Agreement with numpy at every M of the state, in the class the state names; both forms and two runs bit-identical; the pieces of
    solo_pieces bit-identical to their rows in one-piece handles."""
    prob = handle(frx, sc, st)
    try:
        assert prob.P == st.P and prob.Kmax == st.Kmax and list(prob.piece_off) == list(st.piece_off)
        for M in st.Ms:
            assert cs.geometry(M, prob.Kmax) == (st.lpp, 64 // st.lpp), (st.name, M, prob.Kmax)
            got = prob.trajectory_check(st.T, st.Cf, M)
            assert_agrees(got, st.T, st.Cf, st.piece_polys, st.params(sc.ZHANGJIAJIE), M, list(st.piece_off))
            assert same(got, prob.trajectory_check(st.T, st.Cf, M))
            assert np.array_equal(device_rows(prob, st, M), got["piece"])
            for q in solo_pieces:
                assert np.array_equal(solo_row(frx, sc, st, q, M), got["piece"][q]), (st.name, M, q)
    finally:
        prob.close()


@pytest.mark.parametrize("lpp,P", cs.packing_cases(), ids=[f"lpp{lpp}-ppw{64 // lpp}-P{P}" for lpp, P in cs.packing_cases()])
def test_packing_from_M(frx, sc, lpp, P):
    st = cs.packing_state(lpp, P)
    ppw = 64 // lpp
    # the last piece (of a partial wave when P is no multiple of ppw; its neighbour has another K) and one from the middle of the first wave
    solo = sorted({P - 1, min(P - 1, ppw // 2)}) if P in (ppw + 1, 4 * ppw + 1) else ()
    check_geometry_state(frx, sc, st, solo)


@pytest.mark.parametrize("Kmax,Ms", cs.LDS_CASES, ids=[f"Kmax{K}-lpp{cs.geometry(Ms[0], K)[0]}" for K, Ms in cs.LDS_CASES])
def test_packing_from_the_LDS_rule(frx, sc, Kmax, Ms):
    """Kmax = 506 is the capacity edge: 2047 of a wave's 2048 doubles."""
    st = cs.lds_state(Kmax, Ms)
    check_geometry_state(frx, sc, st, (1, st.P - 1) if Kmax in (40, 260, 506) else ())      # (both carry the large polytope; in a one-piece handle lpp comes from M)


def test_capacity_refusal(frx, sc):
    """Kmax = 507 needs 2051 doubles: the check is refused before anything is launched, and the library goes on working."""
    rng = np.random.default_rng(3)
    poly = cs.padded_box(rng, 507)
    T, Cf = cs._quintics(rng, 2)
    st = cs.State("Kmax507", [2], [0, 0], [poly], dict(cs.LOOSE), T, Cf, (1, 64))
    assert cs.geometry(1, 507) is None and cs.geometry(64, 507) is None
    ok = cs.lds_state(40, (1, 3))
    other = handle(frx, sc, ok)
    try:
        prob = handle(frx, sc, st)
    except frx.FrxError as e:                                              # (refused at create: then there is nothing to launch)
        assert e.code == FRX_ERR_CAPACITY
        prob = None
    try:
        if prob is not None:
            assert prob.Kmax == 507
            L = frx.lib()
            t, c = np.ascontiguousarray(st.T), np.ascontiguousarray(st.Cf).reshape(-1)
            for M in st.Ms:
                piece, cand, flags = np.full(16, SENTINEL), np.full(8, SENTINEL), np.full(1, 77, np.uint32)
                assert L.frx_trajectory_check(prob.h, t.ctypes.data, c.ctypes.data, M, piece.ctypes.data, cand.ctypes.data, flags.ctypes.data) == FRX_ERR_CAPACITY
                assert b"507" in L.frx_last_error()
                assert (piece == SENTINEL).all() and (cand == SENTINEL).all() and flags[0] == 77
                with pytest.raises(frx.FrxError) as err:
                    device_rows(prob, st, M)
                assert err.value.code == FRX_ERR_CAPACITY
        got = other.trajectory_check(ok.T, ok.Cf, 3)
        assert_agrees(got, ok.T, ok.Cf, ok.piece_polys, ok.params(sc.ZHANGJIAJIE), 3, list(ok.piece_off))
    finally:
        other.close()
        if prob is not None:
            prob.close()


@pytest.mark.parametrize("moving", [False, True], ids=["point", "line"])
def test_ties_go_to_the_lowest_j_then_k(frx, sc, moving):
    """Every sample of every lane ties on the two copies of the nearest face: (j, k) = (0, 1) has to survive the lane's own loop (M = 200:
    four samples per lane) and every step of the reduction between lanes (M = 7, 63: one sample per lane, lpp = 8 and 64)."""
    st = cs.tie_state(moving, sc.ZHANGJIAJIE)
    prob = handle(frx, sc, st)
    try:
        for M in st.Ms:
            got = prob.trajectory_check(st.T, st.Cf, M)
            row = got["piece"][0]
            assert row[0] == st.expect["value"] and row[6] == 0.0 and row[7] == 1.0, (M, row)
            assert got["candidate"][0, 0] == row[0] and got["candidate"][0, 6] == 0.0 and got["candidate"][0, 7] == 0.0 and got["flags"][0] == 0
            assert np.array_equal(device_rows(prob, st, M)[0], row)
            assert_agrees(got, st.T, st.Cf, st.piece_polys, st.params(sc.ZHANGJIAJIE), M, [0, 1])
    finally:
        prob.close()


def test_equal_pieces_name_the_first(frx, sc):
    st = cs.duplicate_piece_state(sc.ZHANGJIAJIE)
    prob = handle(frx, sc, st)
    try:
        for M in st.Ms:
            got = prob.trajectory_check(st.T, st.Cf, M)
            assert np.array_equal(got["piece"][2], got["piece"][5]) and got["piece"][2, 0] == st.expect["value"]
            assert got["piece"][2, 6] == 0.0 and got["piece"][2, 7] == 1.0
            c = got["candidate"][0]
            assert c[0] == st.expect["value"] and c[7] == st.expect["worst_k"] and c[6] == st.expect["worst_t"], (M, c)
            assert not got["flags"].any()
            assert_agrees(got, st.T, st.Cf, st.piece_polys, st.params(sc.ZHANGJIAJIE), M, list(st.piece_off))
    finally:
        prob.close()


def test_nan_pieces_name_the_first(frx, sc):
    st = cs.nan_order_state(sc.ZHANGJIAJIE)
    prob = handle(frx, sc, st)
    try:
        for M in st.Ms:
            ref_rows, ref_cand, _ = st.reference(sc.ZHANGJIAJIE, M)
            got = prob.trajectory_check(st.T, st.Cf, M)
            for q in st.expect["nan_pieces"]:
                assert np.isnan(got["piece"][q, :6]).all() and got["piece"][q, 6] == 0.0 and got["piece"][q, 7] == 0.0, (M, q, got["piece"][q])
            assert np.array_equal(np.isnan(got["piece"]), np.isnan(ref_rows)) and np.array_equal(np.isnan(got["candidate"]), np.isnan(ref_cand))
            c = got["candidate"][0]
            assert np.isnan(c[:6]).all() and c[7] == st.expect["worst_k"] and c[6] == st.expect["worst_t"], (M, c)
            assert tuple(got["flags"]) == st.expect["flags"]
            assert np.array_equal(device_rows(prob, st, M), got["piece"], equal_nan=True)
    finally:
        prob.close()


def flags_of_state(frx, sc, st, M=cs.FLAG_M):
    prob = handle(frx, sc, st)
    try:
        return prob.trajectory_check(st.T, st.Cf, M)
    finally:
        prob.close()


def test_each_flag_alone_none_and_all(frx, sc):
    states = cs.flag_states(sc.ZHANGJIAJIE)
    loose = flags_of_state(frx, sc, states["none"])
    for name, st in states.items():
        got = flags_of_state(frx, sc, st)
        assert tuple(got["flags"]) == st.expect["flags"], (name, got["flags"])
        assert_agrees(got, st.T, st.Cf, st.piece_polys, st.params(sc.ZHANGJIAJIE), cs.FLAG_M, list(st.piece_off))
        if st.polys is states["none"].polys:
            assert np.array_equal(got["piece"], loose["piece"]) and np.array_equal(got["candidate"], loose["candidate"])    # limits move flags only


def test_flags_are_strict(frx, sc):
    """A limit EQUAL to the value the device reports leaves its bit clear; the next double on the violating side sets it, and only it."""
    loose = flags_of_state(frx, sc, cs.flag_base_state())
    assert not loose["flags"].any()
    for equal, past in cs.strict_states(loose["candidate"][0]):
        bit = equal.expect["bit"]
        a, b = flags_of_state(frx, sc, equal), flags_of_state(frx, sc, past)
        assert np.array_equal(a["candidate"], loose["candidate"]) and np.array_equal(b["candidate"], loose["candidate"])
        assert a["flags"][0] == 0, (equal.name, a["flags"])
        assert b["flags"][0] == bit, (past.name, b["flags"])
    equal, past = cs.corridor_zero_states(sc.ZHANGJIAJIE)
    for M in cs.TIE_M:
        a, b = flags_of_state(frx, sc, equal, M), flags_of_state(frx, sc, past, M)
        assert a["candidate"][0, 0] == 0.0 and a["flags"][0] == 0, (M, a["candidate"][0])
        assert b["candidate"][0, 0] == 2.0 ** -52 and b["flags"][0] == 1, (M, b["candidate"][0])
        for got in (a, b):
            assert got["piece"][0, 6] == 0.0 and got["piece"][0, 7] == 1.0
