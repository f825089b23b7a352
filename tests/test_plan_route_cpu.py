"""Which driver a plan takes and what happens when one gives up (fast-racing_amd/csrc/frx_plan_route.hpp), in its host build (tests/hostcheck).  The decisions
over grids, against the lines of frx_optimize and optimize_device_vectors they replace, restated below in the order they stood there; and the route itself
against drivers played from a script (tests/hostcheck/plan_route_main.cpp): the calls it makes, what it leaves in the caller's arrays, the handle's counters and
the four times.  Nothing expected here is computed by the code under test.  No GPU."""
import ctypes as C
import itertools
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_hostcheck import _load_hostcheck  # noqa: E402

LBERR = list(range(-1024, -1000))            # LBERR_UNKNOWN ... LBERR_INCREASEGRADIENT (frx_lbfgs.hpp)
MINIMUMSTEP, MAXIMUMITERATION, INCREASEGRADIENT = -1007, -1004, -1001
FRX_ERR_HIP = -3
ON = (0, 0, -1, 0, 0, 0, 0)                  # FRX_LBFGS=host, FRX_RESIDENT=0, FRX_RESIDENT_RETRY's first character (-1 unset), FRX_TAKEOVER=0, FRX_RESIDENT_QUEUE=0, spare
HANDLE = dict(lbfgs_mode=0, resident_mode=1, resident_retry=0, takeover_at=0, solver=0, knot_threads=64, mem_size=128)


def _ints(v):
    return np.ascontiguousarray(v, dtype=np.int32)


@pytest.fixture(scope="module")
def hc():
    H = _load_hostcheck()
    ip, dp = np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS"), np.ctypeslib.ndpointer(dtype=np.float64, flags="C_CONTIGUOUS")
    H.hostcheck_plan_route.restype = C.c_int
    H.hostcheck_plan_route.argtypes = [ip, ip, C.c_int, ip, C.c_int, C.c_int, ip, np.ctypeslib.ndpointer(dtype=np.uint32, flags="C_CONTIGUOUS"), ip,
                                       np.ctypeslib.ndpointer(dtype=np.uint8, flags="C_CONTIGUOUS"), dp, dp, ip, C.c_void_p, C.c_void_p, C.c_void_p,
                                       np.ctypeslib.ndpointer(dtype=np.int64, flags="C_CONTIGUOUS"), dp, ip, dp, C.c_int, ip, C.c_char_p, C.c_int]
    for name, args in (("retry_mode", [C.c_int, C.c_int]), ("wants_retry", [C.c_int, C.c_int]), ("resident_first", [ip, C.c_int, C.c_long]),
                       ("wants_device_vectors", [ip, C.c_int]), ("skip_inactive", [C.c_int, C.c_int])):
        getattr(H, "hostcheck_" + name).restype = C.c_int
        getattr(H, "hostcheck_" + name).argtypes = args
    H.hostcheck_takeover_rule.restype = None
    H.hostcheck_takeover_rule.argtypes = [ip] + [C.c_int] * 8 + [C.c_long, np.ctypeslib.ndpointer(dtype=np.int64, flags="C_CONTIGUOUS")]
    H.hostcheck_dv_pre_geometry.restype = None
    H.hostcheck_dv_pre_geometry.argtypes = [C.c_int, C.c_char_p, ip]
    return H


# ---- the decisions ----

def test_retry_mode(hc):
    for env, flag in itertools.product((None, "0", "1", "t", "x", ""), (0, 1)):
        want = (0 if env[:1] == "0" else 2 if env[:1] == "t" else 1) if env is not None else (1 if flag != 0 else 2)
        first = -1 if env is None else (ord(env[0]) if env else 0)          # (an empty value: its first character is the terminator)
        assert hc.hostcheck_retry_mode(first, flag) == want, (env, flag)


def test_wants_retry(hc):
    assert INCREASEGRADIENT in LBERR and MAXIMUMITERATION in LBERR and len(LBERR) == 24
    for st, mode in itertools.product(LBERR + [0, 3], (0, 1, 2)):
        want = st < 0 and st != MAXIMUMITERATION and (mode == 1 or (mode == 2 and st == INCREASEGRADIENT))
        assert hc.hostcheck_wants_retry(st, mode) == int(want), (st, mode)


def test_which_path_comes_first(hc):
    for host, off, mode, lbfgs_mode, at in itertools.product((0, 1), (0, 1), (0, 1, 2), (0, 1), (0, 3)):
        sw = _ints((host, off, -1, 0, 0, 0, 0))
        assert hc.hostcheck_wants_device_vectors(sw, lbfgs_mode) == int(not host and lbfgs_mode != 1)
        assert hc.hostcheck_resident_first(sw, mode, at) == int(not off and mode != 0 and at <= 0)
    for sk, B in itertools.product((-1, 0, 1), (1, 64, 65, 110)):
        assert hc.hostcheck_skip_inactive(sk, B) == int(sk != 0 if sk >= 0 else B > 64)


def test_the_take_over_rule(hc):
    """Every one of the five things that must hold for a take-over to be wanted, off in turn; then the geometry the take-over covers, the shortest vector, the
    chip's capacity against the batch, and the tests' early hand-over."""
    wanted_off = [dict(), dict(takeover_off=1), dict(resident_off=1), dict(queue_off=1), dict(resident_mode=0), dict(gave_up=1)]
    out = np.zeros(3, np.int64)
    n = reached = 0
    for w, solver, kt, m, min_n, cap, B, at in itertools.product(wanted_off, (0, 1), (64, 128), (127, 128), (255, 256), (0, 1, 32), (1, 32, 33, 110), (0, 3)):
        sw = _ints((0, w.get("resident_off", 0), -1, w.get("takeover_off", 0), w.get("queue_off", 0), 0, 0))
        mode, gave_up = w.get("resident_mode", 1), w.get("gave_up", 0)
        # frx_optimize's block, in its order
        capacity, not_before, asked = 0, 1, 0
        wanted = not w.get("takeover_off") and not w.get("resident_off") and not w.get("queue_off") and mode != 0 and not gave_up
        if wanted and solver == 0 and kt == 64 and m == 128:
            asked = 1                                                        # (the device's properties: asked for here and nowhere else)
            fits = min_n >= 2 * m
            if fits and cap >= 1 and B > cap: capacity = cap
            if at > 0:
                not_before = at
                if fits and cap >= 1 and B <= cap: capacity = cap
        hc.hostcheck_takeover_rule(sw, mode, gave_up, solver, kt, m, min_n, cap, B, at, out)
        assert out.tolist() == [capacity, not_before, asked], (w, solver, kt, m, min_n, cap, B, at)
        n += 1; reached += capacity > 0
    assert n == 6 * 2 * 2 * 2 * 2 * 3 * 4 * 2 and reached > 0
    hc.hostcheck_takeover_rule(_ints(ON), 1, 0, 0, 64, 128, 641, -1, 110, 0, out)      # the device could not be asked
    assert out.tolist() == [0, 1, 1]


def _dv_geometry(n):
    best, got = None, (0, 0, 0)
    for e in (8, 6, 4, 2):
        for w in range(1, 9):
            hs = 64 * w * e
            if n <= hs and (best is None or hs < best): best, got = hs, (e, w, 16 if e == 2 else 4 if e == 8 else 8)
    return got


def test_the_direction_kernels_geometry_and_its_override(hc):
    out = np.zeros(4, np.int32)
    for n in (1, 128, 129, 641, 768, 769, 4096, 4097):
        hc.hostcheck_dv_pre_geometry(n, None, out)
        assert out.tolist() == list(_dv_geometry(n)) + [4], n
    e, w = 4, 3
    for n, geom, admitted in ((64 * w * e, b"4,3,5,2", True), (64 * w * e + 1, b"4,3,5,2", False), (64 * w * e, b"4,3,5", False), (64 * w * e, b"4;3;5;2", False),
                              (64 * w * e, b"", False), (10, b"2,1,16,8", True)):
        hc.hostcheck_dv_pre_geometry(n, geom, out)
        want = [int(v) for v in geom.split(b",")] if admitted else list(_dv_geometry(n)) + [4]
        assert out.tolist() == want, (n, geom)


# ---- the route against scripted drivers ----

LENS = (256, 300, 641)


def _x_start(xoff):
    return 0.25 * np.arange(xoff[-1])


def _wrote(k, b, xoff):
    """What the scripted driver's call k leaves for candidate b: x, iters, evals, objective."""
    return 1000.0 * (k + 1) + b + 0.001 * np.arange(xoff[b + 1] - xoff[b]), 100 * (k + 1) + b, 200 * (k + 1) + b, 0.5 + 10.0 * (k + 1) + b


def _times(k):
    return [2.0 ** (4 * k + q) for q in range(4)]


def _route(hc, calls, sw=ON, cap=8, lens=LENS, optional=True, **handle):
    """calls: (rc, device status, [status per candidate], [handed over per candidate] or None) per driver call, whichever driver it is."""
    B = len(lens)
    h = dict(HANDLE, **handle)
    xoff = _ints(np.concatenate([[0], np.cumsum(lens)]))
    n = len(calls)
    rc = _ints([c[0] for c in calls] + [0]); dev = np.ascontiguousarray([c[1] for c in calls] + [0], dtype=np.uint32)
    status = _ints([c[2] for c in calls] + [[0] * B]); hand = np.ascontiguousarray([c[3] or [0] * B for c in calls] + [[0] * B], dtype=np.uint8)
    times = np.ascontiguousarray([_times(k) for k in range(n + 1)], dtype=np.float64)
    x = _x_start(xoff); st = _ints([77] * B); it = _ints([78] * B); ev = _ints([79] * B); obj = np.full(B, 80.0)
    counters = np.array([91, 92, 93, 94, 95, 96, 97, 98, 99, 9], np.int64); stats = np.array([-1.0, -2.0, -3.0, -4.0])
    log = np.zeros((8, 4 + B), np.int32); found = np.zeros((8, B)); made = np.zeros(3, np.int32); err = C.create_string_buffer(256)
    opt = (lambda a: a.ctypes.data) if optional else (lambda a: None)
    ret = hc.hostcheck_plan_route(_ints(sw), _ints([h[k] for k in ("lbfgs_mode", "resident_mode", "resident_retry", "takeover_at", "solver", "knot_threads", "mem_size")]),
                                  B, xoff, cap, n, rc, dev, status, hand, times, x, st, opt(it), opt(ev), opt(obj), counters, stats, log, found, 8, made, err, 256)
    rows = [(("resident", "per_stage")[r[0]], (int(r[2]), int(r[3])) if r[1] else None, None if r[4] < 0 else r[4:].tolist()) for r in log[:made[0]]]
    names = ("resident_used", "resident_retried", "resident_failed", "resident_clusters", "taken_over")
    return SimpleNamespace(ret=ret, calls=rows, found=found[:made[0]], x=x, status=st.tolist(), iters=it.tolist(), evals=ev.tolist(), objective=obj.tolist(), xoff=xoff,
                           counters=dict(zip(names, counters[:5].tolist())), spec=counters[5:9].tolist(), stats=stats.tolist(), cap_asked=int(made[1]), err=(int(made[2]), err.value.decode()))


def _check_outcome(r, source, status):
    """source[b]: the call whose result candidate b must carry, or None for its start point; status: the verdicts."""
    for b, k in enumerate(source):
        seg = slice(r.xoff[b], r.xoff[b + 1])
        if k is None:
            assert np.array_equal(r.x[seg], _x_start(r.xoff)[seg]), b
            continue
        x, it, ev, obj = _wrote(k, b, r.xoff)
        assert np.array_equal(r.x[seg], x) and (r.iters[b], r.evals[b], r.objective[b]) == (it, ev, obj), (b, k)
    assert r.status == status


def _found(r, call, source):
    """the first element of every candidate's x as driver call `call` found it: the result of call source[b], or the start point"""
    want = [_x_start(r.xoff)[r.xoff[b]] if k is None else _wrote(k, b, r.xoff)[0][0] for b, k in enumerate(source)]
    assert r.found[call].tolist() == want, (call, r.found[call].tolist(), want)


def test_resident_plan_that_ends_clean(hc):
    r = _route(hc, [(0, 0, [0, 3, MAXIMUMITERATION], None)])
    assert r.ret == 0 and r.calls == [("resident", None, None)] and r.cap_asked == 0
    _check_outcome(r, [0, 0, 0], [0, 3, MAXIMUMITERATION])
    assert r.counters == dict(resident_used=7, resident_retried=0, resident_failed=0, resident_clusters=3, taken_over=0) and r.spec == [10, 11, 12, 13]
    assert r.stats == _times(0)


@pytest.mark.parametrize("env,flag,again", [(ord("0"), 1, None), (ord("1"), 0, [1, 1, 0]), (-1, 1, [1, 1, 0]), (-1, 0, [1, 0, 0]), (ord("t"), 1, [1, 0, 0])])
@pytest.mark.parametrize("optional", [True, False])
def test_failed_candidates_are_planned_again_per_stage(hc, env, flag, again, optional):
    first = [INCREASEGRADIENT, MINIMUMSTEP, 0]
    second = [0, MINIMUMSTEP, 5]
    r = _route(hc, [(0, 0, first, None), (0, 0, second, None)], sw=(0, 0, env, 0, 0, 0, 0), resident_retry=flag, optional=optional)
    assert r.ret == 0
    if again is None:
        assert r.calls == [("resident", None, None)] and r.counters["resident_retried"] == 0 and r.stats == _times(0)
        return
    assert r.calls == [("resident", None, None), ("per_stage", None, again)]
    _found(r, 1, [None if a else 0 for a in again])                               # who is planned again restarts from its start point, the others keep the resident result
    if optional: _check_outcome(r, [1 if a else 0 for a in again], [second[b] if a else first[b] for b, a in enumerate(again)])
    else: assert r.status == [second[b] if a else first[b] for b, a in enumerate(again)]
    assert r.counters == dict(resident_used=7, resident_retried=sum(again), resident_failed=2, resident_clusters=3, taken_over=0)
    t0, t1 = _times(0), _times(1)
    assert r.stats == [t1[0] + t0[0], t1[1], t1[2], t1[3]]                       # (the wall times add up; device share, host share and rounds are the second run's alone)


def test_a_retry_that_cannot_run_keeps_the_resident_outcome(hc):
    first = [INCREASEGRADIENT, MINIMUMSTEP, 0]
    r = _route(hc, [(0, 0, first, None), (1, 0, [0, 0, 0], None)], resident_retry=1)
    assert r.ret == 0 and r.calls == [("resident", None, None), ("per_stage", None, [1, 1, 0])]
    _check_outcome(r, [0, 0, 0], first)
    assert r.counters == dict(resident_used=7, resident_retried=0, resident_failed=2, resident_clusters=3, taken_over=0)
    assert r.stats == _times(0)


def test_a_retry_that_fails_returns_its_code(hc):
    r = _route(hc, [(0, 0, [INCREASEGRADIENT, 0, 0], None), (-6, 0, [0, 0, 0], None)])
    assert r.ret == -6 and r.calls == [("resident", None, None), ("per_stage", None, [1, 0, 0])]


@pytest.mark.parametrize("cap,take", [(2, (2, 1)), (8, None), (0, None), (-1, None)])
def test_resident_kernel_not_applicable(hc, cap, take):
    """1 without a device status: the per-stage rounds run from the start point (whatever the resident attempt left in x), with a take-over when the batch is larger
    than the chip's capacity."""
    done = [0, MINIMUMSTEP, 3]
    r = _route(hc, [(1, 0, [0, 0, 0], None), (0, 0, done, None)], cap=cap)
    assert r.ret == 0 and r.calls == [("resident", None, None), ("per_stage", take, None)] and r.cap_asked == 1
    _found(r, 1, [None, None, None])
    _check_outcome(r, [1, 1, 1], done)
    assert r.counters == dict(resident_used=0, resident_retried=0, resident_failed=0, resident_clusters=0, taken_over=0) and r.spec == [0, 0, 0, 0]
    assert r.stats == _times(1)


def test_resident_kernel_that_gave_up_is_not_offered_a_take_over(hc):
    r = _route(hc, [(1, 5, [0, 0, 0], None), (0, 0, [0, 0, 0], None)], cap=2)
    assert r.ret == 0 and r.calls == [("resident", None, None), ("per_stage", None, None)] and r.cap_asked == 0
    _found(r, 1, [None, None, None])


def test_stragglers_finish_on_the_resident_kernel(hc):
    """... and the second chance that follows looks at them alone: candidate 0 ended on the per-stage rounds with the same code and is left as it is."""
    ps = [INCREASEGRADIENT, 0, 0]
    res = [0, INCREASEGRADIENT, MINIMUMSTEP]
    again = [0, 3, 0]
    r = _route(hc, [(2, 0, ps, [0, 1, 1]), (0, 0, res, None), (0, 0, again, None)], sw=(0, 0, -1, 0, 0, 0, 0), cap=2, takeover_at=3)
    assert r.ret == 0 and r.calls == [("per_stage", (2, 3), None), ("resident", (2, 3), None), ("per_stage", None, [0, 1, 0])]
    _found(r, 1, [0, None, None])                                                 # (the stragglers' x is still the caller's: their vectors live on the device)
    _found(r, 2, [0, None, 1])
    _check_outcome(r, [0, 2, 1], [INCREASEGRADIENT, 3, MINIMUMSTEP])
    assert r.counters == dict(resident_used=8, resident_retried=1, resident_failed=2, resident_clusters=2, taken_over=2) and r.spec == [20, 21, 22, 23]
    assert r.stats == [a + b + c for a, b, c in zip(_times(0), _times(1), _times(2))]
    # the same without anything to retry: the sums of the two parts
    r = _route(hc, [(2, 0, ps, [0, 1, 1]), (0, 0, [0, 0, MINIMUMSTEP], None)], cap=2, takeover_at=3)
    assert r.ret == 0 and len(r.calls) == 2 and r.counters["taken_over"] == 2 and r.counters["resident_retried"] == 0
    assert r.stats == [a + b for a, b in zip(_times(0), _times(1))]


def test_stragglers_the_resident_kernel_refuses_are_planned_again(hc):
    ps = [3, 0, 0]
    again = [0, 0, MINIMUMSTEP]
    r = _route(hc, [(1, 0, [0, 0, 0], None), (2, 0, ps, [0, 1, 1]), (1, 5, [0, 0, 0], None), (0, 0, again, None)], cap=2)
    assert r.ret == 0 and r.calls == [("resident", None, None), ("per_stage", (2, 1), None), ("resident", (2, 1), None), ("per_stage", None, [0, 1, 1])]
    _found(r, 3, [1, None, None])                                                 # they, and only they, from their start points
    _check_outcome(r, [1, 3, 3], [3, 0, MINIMUMSTEP])
    assert r.counters == dict(resident_used=0, resident_retried=0, resident_failed=0, resident_clusters=0, taken_over=0)
    assert r.stats == [a + b for a, b in zip(_times(1), _times(3))]
    # a second refusal
    r = _route(hc, [(1, 0, [0, 0, 0], None), (2, 0, ps, [0, 1, 1]), (1, 0, [0, 0, 0], None), (1, 0, again, None)], cap=2)
    assert r.ret == FRX_ERR_HIP and r.err == (FRX_ERR_HIP, "per-stage path unavailable after a failed take-over") and len(r.calls) == 4
    r = _route(hc, [(1, 0, [0, 0, 0], None), (2, 0, ps, [0, 1, 1]), (1, 0, [0, 0, 0], None), (-6, 0, again, None)], cap=2)
    assert r.ret == -6 and r.err == (0, "")
    r = _route(hc, [(1, 0, [0, 0, 0], None), (2, 0, ps, [0, 1, 1]), (-7, 0, [0, 0, 0], None)], cap=2)
    assert r.ret == -7 and len(r.calls) == 3


def test_an_early_hand_over_skips_the_resident_first_attempt(hc):
    r = _route(hc, [(0, 0, [0, 0, 0], None)], cap=8, takeover_at=3)
    assert r.ret == 0 and r.calls == [("per_stage", (8, 3), None)]
    r = _route(hc, [(0, 0, [0, 0, 0], None)], cap=0, takeover_at=3)
    assert r.ret == 0 and r.calls == [("per_stage", None, None)]


@pytest.mark.parametrize("sw,lbfgs_mode", [((1, 0, -1, 0, 0, 0, 0), 0), (ON, 1)])
def test_host_vectors_asked_for(hc, sw, lbfgs_mode):
    r = _route(hc, [], sw=sw, lbfgs_mode=lbfgs_mode)
    assert r.ret == 1 and r.calls == []
    _check_outcome(r, [None, None, None], [77, 77, 77])
    assert r.counters == dict(resident_used=91, resident_retried=92, resident_failed=93, resident_clusters=94, taken_over=0) and r.stats == [-1.0, -2.0, -3.0, -4.0]


def test_no_device_path_runs(hc):
    r = _route(hc, [(1, 0, [0, 0, 0], None), (1, 0, [0, 0, 0], None)])
    assert r.ret == 1 and r.calls == [("resident", None, None), ("per_stage", None, None)]
    _check_outcome(r, [None, None, None], [0, 0, 0])                              # (the resident attempt cleared the verdicts; x is the start point again)
    r = _route(hc, [(1, 0, [0, 0, 0], None)], sw=(0, 1, -1, 0, 0, 0, 0))
    assert r.ret == 1 and r.calls == [("per_stage", None, None)] and r.cap_asked == 0
