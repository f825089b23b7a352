"""The edge states of the dense feasibility check (tests/check_states.py) without a device: every builder runs with its self-checks, the numpy
restatement gives the stated answers on the tie, NaN and flag states, and the restated geometry rule names the classes the GPU tests rely on."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import check_reference as cr  # noqa: E402
import check_states as cs  # noqa: E402


def test_geometry_rule():
    assert cs.geometry(1, 5) == (2, 32) and cs.geometry(1, 40) == (8, 8) and cs.geometry(1, 260) == (64, 1) and cs.geometry(1, 507) is None
    assert cs.geometry(1, 506) == (64, 1) and cs.geometry(64, 506) == (64, 1) and cs.geometry(16384, 507) is None
    assert cs.wave_lds(1, 506) == 2047 and cs.wave_lds(1, 507) == 2051
    # M alone: the smallest power of two that holds M + 1 samples, 2 .. 64
    for M, lpp in ((1, 2), (2, 4), (3, 4), (4, 8), (7, 8), (8, 16), (15, 16), (16, 32), (31, 32), (32, 64), (63, 64), (64, 64), (16384, 64)):
        assert cs.geometry(M, 1) == (lpp, 64 // lpp)
    # the LDS rule: each class ends at k_cap
    assert [cs.k_cap(lpp) for lpp in (2, 4, 8, 16, 32, 64)] == [10, 26, 58, 122, 250, 506]
    for lpp in (2, 4, 8, 16, 32):
        assert cs.geometry(1, cs.k_cap(lpp)) == (lpp, 64 // lpp) and cs.geometry(1, cs.k_cap(lpp) + 1) == (2 * lpp, 32 // lpp)


@pytest.mark.parametrize("lpp", [2, 4, 8, 16, 32, 64])
def test_packing_states(lpp):
    ppw = 64 // lpp
    counts = cs.packing_counts(ppw)
    assert counts[0] == 1 and counts[-1] == 4 * ppw + 1
    for P in counts:
        st = cs.packing_state(lpp, P)
        assert st.P == P and st.lpp == lpp and f"lpp{lpp}-" in st.name and st.Kmax <= 40
        assert lpp in (st.Ms[0] + 1, 64) and (lpp == 2 or st.Ms[1] + 1 < lpp)     # one M fills the group, one leaves it short
    if lpp == 64:
        assert {65, 127, 129} <= set(cs.M_OF[64])
    assert (lpp, 4 * ppw + 1) in cs.packing_cases()
    rows, cand, flags = cs.packing_state(lpp, ppw + 1).reference(SC(), cs.M_OF[lpp][0])
    assert np.isfinite(rows).all() and np.isfinite(cand).all() and not (flags & 30).any()


def SC():
    """The stock parameters the GPU tests build their handles from."""
    import frx_import  # noqa: F401  (registers the package under its importable name)
    from fast_racing_amd import scenario
    return scenario.ZHANGJIAJIE


def test_lds_states(frx):
    classes = {}
    for Kmax, Ms in cs.LDS_CASES:
        st = cs.lds_state(Kmax, Ms)
        classes.setdefault(st.lpp, []).append(Kmax)
        assert st.P == 4 * (64 // st.lpp) + 1 and st.Kmax == Kmax and st.piece_polys[1].shape[1] == Kmax and st.piece_polys[-1].shape[1] == Kmax
    assert classes == {4: [11, 26], 8: [27, 40, 58], 16: [59, 122], 32: [123, 250], 64: [251, 260, 506]}
    rows, cand, flags = cs.lds_state(40, (1, 3)).reference(SC(), 3)
    assert np.isfinite(rows).all() and not (flags & 30).any()


def test_tie_states(frx):
    base = SC()
    for moving in (False, True):
        st = cs.tie_state(moving, base)
        for M in st.Ms:
            rows, cand, flags = st.reference(base, M)
            assert rows[0, 0] == -0.125 and rows[0, 6] == 0.0 and rows[0, 7] == 1.0
            assert cand[0, 0] == -0.125 and cand[0, 6] == 0.0 and cand[0, 7] == 0.0 and flags[0] == 0
            assert rows[0, 1] == (np.hypot(0.5, 0.25) if moving else 0.0) and rows[0, 2] == rows[0, 3] == 8.0 and rows[0, 4] == 0.0
    st = cs.duplicate_piece_state(base)
    rows, cand, flags = st.reference(base, 7)
    assert cr.reduce_candidates(rows, st.T, st.piece_off)[0, 7] == 2.0 and cand[0, 6] == st.expect["worst_t"] == 0.75
    # the reduction keeps the FIRST of equal pieces whatever their order: swap the copies' rows and nothing changes
    swapped = rows.copy()
    swapped[[2, 5]] = rows[[5, 2]]
    assert np.array_equal(cr.reduce_candidates(swapped, st.T, st.piece_off), cand)


def test_nan_order_state(frx):
    base = SC()
    st = cs.nan_order_state(base)
    rows, cand, flags = st.reference(base, 63)
    assert tuple(flags) == st.expect["flags"] and cand[0, 7] == 3.0 and cand[0, 6] == 1.75
    # a NaN piece is first whatever follows it: a later piece with a larger finite reach does not displace it
    rows2 = rows.copy()
    rows2[7, 0] = 5.0
    c2 = cr.reduce_candidates(rows2, st.T, st.piece_off)
    assert np.isnan(c2[0, 0]) and c2[0, 7] == 3.0


def test_flag_states(frx):
    base = SC()
    states = cs.flag_states(base)
    assert set(states) == {"none", "vel_max", "thr_acc_min", "thr_acc_max", "body_rate_max", "corridor", "all"}
    got = {name: tuple(int(f) for f in st.reference(base, cs.FLAG_M)[2]) for name, st in states.items()}
    assert got == {"none": (0, 0), "vel_max": (2, 2), "thr_acc_min": (4, 4), "thr_acc_max": (8, 8), "body_rate_max": (16, 16), "corridor": (1, 1),
                   "all": (31, 31)}
    # strictness of the restatement's own comparisons, on its own values
    cand = states["none"].reference(base, cs.FLAG_M)[1]
    for equal, past in cs.strict_states(cand[0]):
        bit = equal.expect["bit"]
        assert not equal.reference(base, cs.FLAG_M)[2][0] & bit and past.reference(base, cs.FLAG_M)[2][0] & bit
        assert past.reference(base, cs.FLAG_M)[2][0] == bit                 # and nothing else
    equal, past = cs.corridor_zero_states(base)
    for M in cs.TIE_M:
        assert equal.reference(base, M)[1][0, 0] == 0.0 and equal.reference(base, M)[2][0] == 0
        assert past.reference(base, M)[1][0, 0] == 2.0 ** -52 and past.reference(base, M)[2][0] == 1
