"""The host's side of the resident kernel's mailbox protocol (fast-racing_amd/csrc/frx_resident_mailbox.hpp) without a device: in tests/hostcheck/resident_mailbox_main.cpp
a plain thread plays the clusters over ordinary host memory - it reads each command word, executes the command on a host emulation of the device vectors (a small
quadratic per candidate), answers with the result and the command's sequence number, and honours DV_NEXT and DV_QUIT.  Whichever cluster runs a candidate, and
whether the caller alone or two threads serve the mailboxes, its plan must be the one the same solver makes with nobody in between; every cluster is told to quit
exactly once, also when the plan is aborted.  No GPU."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_hostcheck import _load_hostcheck  # noqa: E402

NORMAL, INVALID, TAKEOVER, GIVES_UP, SILENT_LEFT, SILENT_TIMEOUT = range(6)
NOTHING = -77                        # what the harness leaves where the mailbox recorded nothing
LBERR_INVALID_N = -1021


@pytest.fixture(scope="module")
def hc():
    H = _load_hostcheck()
    ip = np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS")
    dp = np.ctypeslib.ndpointer(dtype=np.float64, flags="C_CONTIGUOUS")
    H.hostcheck_resident_mailbox_case.restype = C.c_int
    H.hostcheck_resident_mailbox_case.argtypes = [C.c_int] * 5 + [C.c_double, C.c_int, ip, ip, ip, dp, dp, ip, ip]
    return H


def _case(hc, S, B, nsrv, mode=NORMAL, arg=0, timeout_ms=2000.0, stride=4):
    r = {"status": np.zeros(B, np.int32), "iters": np.zeros(B, np.int32), "evals": np.zeros(B, np.int32), "objective": np.zeros(B), "solo": np.zeros((B, 4)),
         "next": np.zeros(B, np.int32), "quits": np.zeros(S, np.int32)}
    r["abort"] = hc.hostcheck_resident_mailbox_case(S, B, nsrv, mode, arg, timeout_ms, stride, r["status"], r["iters"], r["evals"], r["objective"], r["solo"], r["next"], r["quits"])
    return r


def _same_as_alone(r, cands):
    for b in cands:
        assert (r["status"][b], r["iters"][b], r["evals"][b], r["objective"][b]) == tuple(r["solo"][b]), (b, r)


@pytest.mark.parametrize("S,B,nsrv,stride", [(1, 1, 1, 4), (2, 5, 1, 4), (2, 5, 2, 4), (2, 5, 2, 1), (3, 3, 3, 4)])
def test_every_candidate_is_planned_once_whichever_cluster_runs_it(hc, S, B, nsrv, stride):
    r = _case(hc, S, B, nsrv, stride=stride)
    assert r["abort"] == 0 and r["quits"].tolist() == [1] * S
    assert r["next"].tolist() == [0] * S + [1] * (B - S)            # the first S start on their clusters, every other one is handed over exactly once
    _same_as_alone(r, range(B))
    assert (r["status"] == 0).all() and (r["iters"] > 3).all() and (r["objective"] < 1e-8).all()   # (the quadratics converge: real plans went through the mailbox)


@pytest.mark.parametrize("nsrv,invalid", [(1, 0), (2, 1), (1, 3), (2, 4)])
def test_a_candidate_with_nothing_to_run_is_handed_over_at_once(hc, nsrv, invalid):
    """Invalid parameters (no variables): the first command is empty - on a cluster's first candidate and on one that comes through the queue."""
    r = _case(hc, 2, 5, nsrv, INVALID, invalid)
    assert r["abort"] == 0 and r["quits"].tolist() == [1, 1]
    assert r["next"].tolist() == [0, 0, 1, 1, 1]
    assert r["status"][invalid] == LBERR_INVALID_N and r["evals"][invalid] == 0
    _same_as_alone(r, range(5))
    assert (np.delete(r["status"], invalid) == 0).all()


@pytest.mark.parametrize("after", [1, 3, 6])
def test_a_take_over_continues_pending_commands_and_hands_nobody_on(hc, after):
    r = _case(hc, 2, 5, 1, TAKEOVER, after)
    assert r["abort"] == 0 and r["quits"].tolist() == [1, 1]
    assert r["next"].tolist() == [0] * 5                             # next_cand = B: no DV_NEXT at all
    _same_as_alone(r, (1, 3))
    assert (r["status"][[1, 3]] == 0).all()
    assert (r["status"][[0, 2, 4]] == NOTHING).all() and (r["objective"][[0, 2, 4]] == NOTHING).all()   # everybody else's results are left alone


@pytest.mark.parametrize("mode,nsrv,odd,timeout_ms,code", [(GIVES_UP, 1, 1, 2000.0, 1), (GIVES_UP, 2, 0, 2000.0, 1), (SILENT_LEFT, 1, 1, 2000.0, 1), (SILENT_TIMEOUT, 1, 0, 50.0, 2),
                                                           (SILENT_TIMEOUT, 2, 1, 50.0, 2)])
def test_an_aborted_plan_still_tells_every_cluster_to_quit(hc, mode, nsrv, odd, timeout_ms, code):
    """A cluster that writes ~0 (the device gave up): 1.  A silent cluster: 1 when the kernel has left (thread 0's probe, while it has a cluster waiting), 2 after the timeout."""
    r = _case(hc, 2, 5, nsrv, mode, odd, timeout_ms)
    assert r["abort"] == code
    assert r["quits"].tolist() == [1, 1]
