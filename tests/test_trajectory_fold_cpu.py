"""The host fold of frx_trajectory_check / _extrema / _clearance (piece rows -> candidate rows and flag words, fast-racing_amd/csrc/frx_traj_fold.hpp),
reached without a device through frx_debug_fold_rows, against the Python restatements the GPU tests use (check_reference, extrema_reference,
clear_reference): exact equality, NaNs by position, on the hand-made rows of tests/fold_cases.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import check_reference as cr  # noqa: E402
import clear_reference as clr  # noqa: E402
import extrema_reference as er  # noqa: E402
import fold_cases as fc  # noqa: E402

REDUCE = {0: cr.reduce_candidates, 1: er.reduce_candidates, 2: clr.reduce_candidates}
FLAGS = {0: lambda c: cr.flags_of(c, fc.LIMITS), 1: lambda c: er.flags_of(c, fc.LIMITS), 2: clr.flags_of}


def fold(frx, kind, rows, T=fc.T, poff=fc.POFF, want_cand=True, want_flags=True):
    """frx_debug_fold_rows: (candidate rows or None, flags or None)"""
    B, fields = len(poff) - 1, fc.KINDS[kind]["fields"]
    po = np.ascontiguousarray(poff, dtype=np.int32); T = np.ascontiguousarray(T, dtype=np.float64)
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    cand = np.full((B, fields), -7.0) if want_cand else None
    flags = np.full(B, 0xdead, np.uint32) if want_flags else None
    rc = frx.lib().frx_debug_fold_rows(kind, B, po.ctypes.data, T.ctypes.data, rows.ctypes.data, fc.LIMITS4.ctypes.data,
                                       cand.ctypes.data if want_cand else None, flags.ctypes.data if want_flags else None)
    assert rc == 0, frx.lib().frx_last_error()
    return cand, flags


def prefix(b, local):
    """start of a candidate's piece from the candidate's start, summed left to right"""
    t0 = 0.0
    for q in range(local):
        t0 += float(fc.T[fc.POFF[b] + q])
    return t0


def test_entry_is_exported_and_checks_its_arguments(frx):
    L = frx.lib()
    assert "frx_debug_fold_rows" in frx.DEBUG_SYMBOLS
    po = np.array(fc.POFF, np.int32); rows = fc.base_rows(0); out = np.zeros((3, 8))
    p, t, r, lim, o = po.ctypes.data, fc.T.ctypes.data, rows.ctypes.data, fc.LIMITS4.ctypes.data, out.ctypes.data
    for bad in (-1, 3):
        assert L.frx_debug_fold_rows(bad, 3, p, t, r, lim, o, None) == -1
    assert L.frx_debug_fold_rows(0, 0, p, t, r, lim, o, None) == -1
    for args in ((None, t, r, lim), (p, None, r, lim), (p, t, None, lim), (p, t, r, None)):
        assert L.frx_debug_fold_rows(0, 3, *args, o, None) == -1
    assert not out.any()
    assert L.frx_debug_fold_rows(0, 3, p, t, r, lim, None, None) == 0            # nothing asked for: nothing done


@pytest.mark.parametrize("kind", sorted(fc.KINDS))
def test_fold_equals_the_restatement(frx, kind):
    names = []
    for name, rows in fc.cases(kind):
        cand, flags = fold(frx, kind, rows)
        want = REDUCE[kind](rows, fc.T, fc.POFF)
        assert np.array_equal(cand, want, equal_nan=True), (name, cand, want)
        assert np.array_equal(flags, FLAGS[kind](want)), (name, flags, FLAGS[kind](want))
        # the optional outputs: flags alone, candidate rows alone
        only_c, none_f = fold(frx, kind, rows, want_flags=False)
        none_c, only_f = fold(frx, kind, rows, want_cand=False)
        assert none_f is None and none_c is None
        assert np.array_equal(only_c, cand, equal_nan=True) and np.array_equal(only_f, flags), name
        names.append(name)
    k = fc.KINDS[kind]
    assert len(names) == 1 + 7 * k["fields"] + 4 * len(k["ranges"]) + 3 * len(k["limits"])


@pytest.mark.parametrize("kind", sorted(fc.KINDS))
def test_flags_are_strict_and_name_non_finite_fields(frx, kind):
    k = fc.KINDS[kind]
    seen = 0
    for name, rows in fc.cases(kind):
        _, flags = fold(frx, kind, rows)
        want = fc.expected_flags_at_limits(kind, name)
        if want is not None:
            assert tuple(int(v) for v in flags) == want, (name, flags)
            seen += 1
        if name == "base":
            assert not flags.any()
    assert seen == 3 * len(k["limits"])
    base = fc.base_rows(kind)
    for f in range(k["fields"]):
        for bad in (np.nan, np.inf, -np.inf):
            rows = base.copy()
            rows[0, f] = bad                                                  # the single piece: its row is the candidate's
            cand, flags = fold(frx, kind, rows)
            if kind == 0 and f == 7:                                          # the check's candidate row names a PIECE there: the rows' half-space index never reaches it
                assert cand[0, 7] == 0.0 and not flags.any()
                continue
            assert flags[0] & k["nonfinite"] and not flags[1] and not flags[2], (f, bad, flags)
            n = 7 if kind == 0 else k["fields"]
            assert np.array_equal(cand[0, :n], rows[0, :n], equal_nan=True) and (kind != 0 or cand[0, 7] == 0.0)


@pytest.mark.parametrize("kind", sorted(fc.KINDS))
def test_first_of_a_tie_wins_with_its_time_from_the_start(frx, kind):
    """Written down without any fold: the candidate of four pieces, pieces 1 and 3 (then 2 and 3, then all) tied for the worst value of a field, and the worst in the
    last piece, whose time rides on (T3 + T4) + T5."""
    k = fc.KINDS[kind]
    by_name = dict(fc.cases(kind))
    for f in range(len(k["ranges"])):
        for name, local in ((f"tie_13_f{f}", 1), (f"tie_23_f{f}", 2), (f"tie_all_f{f}", 0), (f"worst_last_f{f}", 3)):
            rows = by_name[name]
            cand, _ = fold(frx, kind, rows)
            gp = fc.POFF[2] + local
            assert cand[2, f] == rows[gp, f], (name, cand[2])
            if kind == 0 and f == 0:
                assert cand[2, 6] == prefix(2, local) + rows[gp, 6] and cand[2, 7] == float(local), (name, cand[2])
            elif kind == 1:
                assert cand[2, 5 + f] == prefix(2, local) + rows[gp, 5 + f], (name, cand[2])
            elif kind == 2 and f == 0:
                assert cand[2, 2] == prefix(2, local) + rows[gp, 2] and cand[2, 3] == rows[gp, 3], (name, cand[2])
    assert prefix(2, 3) == (0.1 + 0.2) + 0.3 != 0.1 + (0.2 + 0.3)


def test_a_running_nan_stays(frx):
    """The first NaN of a field is the one the candidate reports: its piece and time for the check's reach and the clearance, its time for the extrema."""
    for kind, f, carried in ((0, 0, (6,)), (1, 3, (8,)), (2, 0, (2, 3))):
        rows = dict(fc.cases(kind))[f"nan_twice_f{f}"]
        cand, flags = fold(frx, kind, rows)
        gp = fc.POFF[2] + 1
        assert np.isnan(cand[1, f]) and np.isnan(cand[2, f]) and flags[1] & fc.KINDS[kind]["nonfinite"]
        assert cand[2, carried[0]] == prefix(2, 1) + rows[gp, carried[0]]
        if kind == 0:
            assert cand[2, 7] == 1.0 and cand[1, 7] == 0.0
        if kind == 2:
            assert cand[2, 3] == rows[gp, 3]
