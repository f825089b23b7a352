"""Which kernel form a launch takes (fast-racing_amd/csrc/frx_launch_forms.hpp), in its host build (tests/hostcheck), over every input: the launchers and the
diagnostics that report a form all ask these functions, so what is pinned here is what runs.  Each decision is checked against the ladder of tests the launchers
carried before the header existed, written out below as tables; nothing here is computed by the code under test.  No GPU."""
import ctypes as C
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_hostcheck import _load_hostcheck  # noqa: E402

K16 = 1
# launch_eval_cluster's ladder, first rung that holds wins.  Conditions over the EFFECTIVE switches (handoff = H and A and T, chain = C and handoff,
# geom_on = G and handoff and E, cls = geom_on and the handle is of the geometry class); "E" in a form stands for the raw FRX_EVAL_EARLY_T.
#   (condition, (ARGP, ET, TAIL, HO, CH, GEO))
LADDER = [
    (lambda s: s["cls"] and s["chain"] and not s["stamped"], (1, 1, 1, 1, 1, K16)),
    (lambda s: s["cls"], (1, 1, 1, 1, 0, K16)),
    (lambda s: s["chain"] and not s["stamped"], (1, "E", 1, 1, 1, 0)),
    (lambda s: s["handoff"], (1, "E", 1, 1, 0, 0)),
    (lambda s: s["A"] and s["E"] and not s["T"], (1, 1, 0, 0, 0, 0)),
    (lambda s: s["A"], (1, "E", 1, 0, 0, 0)),
    (lambda s: True, (0, "E", 1, 0, 0, 0)),
]
INPUTS = [(sw, cls, st) for sw in itertools.product((0, 1), repeat=6) for cls in (0, 1) for st in (0, 1)]

# launch_penalty's tests in their order -> (form, what frx_debug_penalty_kernel reports); lat2 stands for the instantiation of the geometry
THR, LAT, LAT2_17, LAT2_49, LAT2_0, LAT2_R5 = range(6)
PENALTY = [
    (lambda forced, pen2, tp: forced != 2 and pen2 and tp == "5", LAT2_R5, 2),
    (lambda forced, pen2, tp: forced != 2 and pen2 and tp != "0", "lat2", 2),
    (lambda forced, pen2, tp: forced != 2, LAT, 1),
    (lambda forced, pen2, tp: True, THR, 0),
]
LAT2_OF = {17: LAT2_17, 49: LAT2_49, 33: LAT2_0}

CLUSTER, SOLO, STAGES = range(3)


@pytest.fixture(scope="module")
def hc():
    H = _load_hostcheck()
    ip = np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS")
    H.hostcheck_eval_cluster_form.restype = C.c_int
    H.hostcheck_eval_cluster_form.argtypes = [ip, C.c_int, C.c_int, C.c_int, ip]
    H.hostcheck_eval_cluster_raised.restype = C.c_int
    H.hostcheck_eval_cluster_raised.argtypes = [ip, ip]
    H.hostcheck_penalty_form.restype = C.c_int
    H.hostcheck_penalty_form.argtypes = [C.c_int] * 4 + [C.POINTER(C.c_int)]
    H.hostcheck_eval_route.restype = C.c_int
    H.hostcheck_eval_route.argtypes = [ip]
    H.hostcheck_pen_wave_doubles.restype = C.c_int
    H.hostcheck_pen_wave_doubles.argtypes = [C.c_int, C.c_int]
    H.hostcheck_pen_wg_bytes.restype = C.c_longlong
    H.hostcheck_pen_wg_bytes.argtypes = [C.c_int] * 4
    lp = np.ctypeslib.ndpointer(dtype=np.int64, flags="C_CONTIGUOUS")
    H.hostcheck_lds_limits.restype = None
    H.hostcheck_lds_limits.argtypes = [C.c_int, ip, ip, lp, ip, lp, ip]
    return H


def _form(hc, sw, cls, stamped, have_dev=1):
    out = np.zeros(6, np.int32)
    ok = hc.hostcheck_eval_cluster_form(np.array(sw, np.int32), cls, stamped, have_dev, out)
    return ok, tuple(int(v) for v in out)


def _raised(hc, sw):
    out = np.full(24, -1, np.int32)
    n = hc.hostcheck_eval_cluster_raised(np.array(sw, np.int32), out)
    assert 1 <= n <= 4
    return [tuple(int(v) for v in out[6 * i:6 * i + 6]) for i in range(n)]


def _table_form(sw, cls, stamped):
    A, E, T, H, Cc, G = sw
    handoff = H and A and T
    s = {"A": A, "E": E, "T": T, "handoff": handoff, "chain": Cc and handoff, "cls": G and handoff and E and cls, "stamped": stamped}
    for cond, form in LADDER:
        if cond(s):
            return tuple(E if v == "E" else v for v in form)


def test_the_ladder_of_the_one_launch_evaluation(hc):
    """All 64 switch settings x class x stamped: the form is the one the ladder gave; without a device block only the by-value form launches."""
    for sw, cls, st in INPUTS:
        want = _table_form(sw, cls, st)
        ok, got = _form(hc, sw, cls, st)
        assert ok == 1 and got == want, (sw, cls, st)
        ok0, got0 = _form(hc, sw, cls, st, have_dev=0)
        assert got0 == want and ok0 == (0 if want[0] else 1), (sw, cls, st)
    # the quirk that stays: FRX_EVAL_TAIL=0 shows only with the argument pointer AND early durations
    assert all(_table_form(sw, cls, st)[2] == 1 for sw, cls, st in INPUTS if not (sw[0] and sw[1]))
    assert {_table_form(sw, cls, st) for sw, cls, st in INPUTS} == {
        (1, 1, 1, 1, 1, K16), (1, 1, 1, 1, 0, K16), (1, 1, 1, 1, 1, 0), (1, 0, 1, 1, 1, 0), (1, 1, 1, 1, 0, 0), (1, 0, 1, 1, 0, 0), (1, 1, 0, 0, 0, 0),
        (1, 1, 1, 0, 0, 0), (1, 0, 1, 0, 0, 0), (0, 1, 1, 0, 0, 0), (0, 0, 1, 0, 0, 0)}, "the eleven instantiations, no other"


def test_every_form_a_launch_takes_has_had_its_limit_raised(hc):
    """The property the launcher kept by hand: for every input the form is in the list raised under the same switches.  And the list holds nothing that no input
    reaches - but, with the chain on, the stamped twin of the unstamped pick (the diagnostics' form), which the inputs here reach too."""
    for sw in itertools.product((0, 1), repeat=6):
        raised = _raised(hc, sw)
        assert len(set(raised)) == len(raised), sw
        reached = set()
        for cls in (0, 1):
            for st in (0, 1):
                f = _table_form(sw, cls, st)
                assert f in raised, (sw, cls, st, f, raised)
                reached.add(f)
        A, E, T, H, Cc, G = sw
        twin = {(1, E, 1, 1, 0, 0)} if (Cc and H and A and T) else set()
        assert set(raised) - reached <= twin, (sw, raised)
        assert _table_form(sw, 0, 0) == raised[0], "the unstamped run-time pick: the form the occupancy query asks about"


def test_penalty_form(hc):
    for pen2, lpp, forced, tp in itertools.product((0, 4096), (17, 49, 33), (0, 1, 2), (None, "0", "1", "5")):
        form, code = next((f, c) for cond, f, c in PENALTY if cond(forced, pen2, tp))
        if form == "lat2":
            form = LAT2_OF[lpp]
        got_code = C.c_int(-1)
        got = hc.hostcheck_penalty_form(pen2, lpp, forced, ord(tp) if tp else 0, C.byref(got_code))
        assert (got, got_code.value) == (form, code), (pen2, lpp, forced, tp)
        # frx_debug_penalty_kernel's own rule
        assert got_code.value == (0 if forced == 2 else 2 if (pen2 and tp != "0") else 1)


def _route_in_launch_eval_order(backward, tap, cand_active, stamps, fused, fused_stamps, solo, B, lo, hi, lds_solo, knot):
    solo_ok = backward and lds_solo and knot and (not stamps or solo == 2)
    if solo_ok and solo == 2:
        return SOLO
    if backward and fused and knot and not tap and not cand_active and (not stamps or fused_stamps):
        return CLUSTER
    if solo_ok and solo == 1 and lo <= B <= hi:
        return SOLO
    return STAGES


def test_eval_route(hc):
    lo, hi = 384, 512
    for bits in itertools.product((0, 1), repeat=8):
        backward, tap, cand_active, stamps, fused, fused_stamps, lds_solo, knot = bits
        for solo in (0, 1, 2):
            for B in (lo - 1, lo, hi, hi + 1):
                args = (backward, tap, cand_active, stamps, fused, fused_stamps, solo, B, lo, hi, lds_solo, knot)
                got = hc.hostcheck_eval_route(np.array(args, np.int32))
                assert got == _route_in_launch_eval_order(*args), args
                if backward and not (tap or cand_active or stamps):
                    # a plain evaluation: frx_debug_eval_solo's condition, as it stood
                    takes_solo = bool(lds_solo and knot and (solo == 2 or (solo == 1 and lo <= B <= hi)) and not (fused and solo != 2))
                    assert (got == SOLO) == takes_solo, args


def test_pen_wave_doubles(hc):
    assert hc.hostcheck_pen_wave_doubles(3, 8) == 1509
    for ppw, kmax in ((3, 8), (7, 8), (1, 14)):
        assert hc.hostcheck_pen_wave_doubles(ppw, kmax) == ppw * 19 + ppw * (kmax + 1) * 4 + 64 * 21
    for ppg, kmax, waves in ((15, 8, 4), (3, 8, 1), (5, 14, 4)):
        for per_lane in (21, 11):
            assert hc.hostcheck_pen_wg_bytes(ppg, kmax, waves, per_lane) == 8 * (ppg * 19 + ppg * (kmax + 1) * 4 + 64 * waves * per_lane)


def _limits(hc, script):
    """script: (device, function, bytes, setter fails) per raise on ONE fresh table -> [(bytes the setter was asked for, 0 = no call; return value)]"""
    dev, fn, byts, fail = (np.array([row[k] for row in script], np.int64 if k == 2 else np.int32) for k in range(4))
    called, rc = np.full(len(script), -7, np.int64), np.full(len(script), -7, np.int32)
    hc.hostcheck_lds_limits(len(script), dev, fn, byts, fail, called, rc)
    return [(int(c), int(r)) for c, r in zip(called, rc)]


def test_a_kernels_lds_limit_only_grows(hc):
    """The table behind raise_lds_limit (LdsLimits) with a setter that only records: what every launcher - k_dilate and k_round, which used to set their limit on every
    launch, among them - now does.  A large need, a small one, the large one again: ONE call, for the large need; the small one never reaches the setter, so it cannot
    lower the limit under a launch in flight, and a later launch with a need already held makes no call at all (it may be inside a stream capture)."""
    big, small, bigger = 96 * 1024 + 1016, 2048, 160 * 1024
    assert _limits(hc, [(0, 0, big, 0), (0, 0, small, 0), (0, 0, big, 0)]) == [(big, 0), (0, 0), (0, 0)]
    # the other order: every step up is a call, for exactly that need
    assert _limits(hc, [(0, 0, small, 0), (0, 0, big, 0), (0, 0, small, 0), (0, 0, bigger, 0), (0, 0, big, 0)]) == [(small, 0), (big, 0), (0, 0), (bigger, 0), (0, 0)]
    # per function and per device: what one holds says nothing about another
    assert _limits(hc, [(0, 0, big, 0), (0, 1, small, 0), (1, 0, small, 0), (0, 1, small, 0), (1, 0, small, 0)]) == [(big, 0), (small, 0), (small, 0), (0, 0), (0, 0)]
    # a refused call is reported and holds nothing: the next launch asks again
    assert _limits(hc, [(0, 0, big, 1), (0, 0, big, 0), (0, 0, big, 0)]) == [(big, 1), (big, 0), (0, 0)]
    assert _limits(hc, [(0, 0, small, 0), (0, 0, big, 1), (0, 0, small, 0), (0, 0, big, 0)]) == [(small, 0), (big, 1), (0, 0), (big, 0)]
    # no need, no call and no error (a form that does not apply to the geometry)
    assert _limits(hc, [(0, 0, 0, 1), (0, 0, small, 0)]) == [(0, 0), (small, 0)]
