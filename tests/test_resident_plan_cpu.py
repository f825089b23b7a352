"""The geometry of a resident plan and the command word (fast-racing_amd/csrc/frx_resident_plan.hpp), in its host build (tests/hostcheck), over a grid of inputs:
optimize_resident and the take-over threshold of frx_optimize both ask these functions, so what is pinned here is what runs.  The expectation is the arithmetic
the driver carried before the header existed, written out below in numpy in the order it stood there; nothing here is computed by the code under test.  No GPU."""
import ctypes as C
import itertools
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_hostcheck import _load_hostcheck  # noqa: E402

ROUND_E, ROUND_E_SMALL, WORDS_PER_CAND = 56, 28, 128
DV_EVAL, DV_INIT, DV_ADVANCE, DV_TRIAL, DV_RESTORE, DV_NEXT, DV_STEP_IS_ONE, DV_QUIT = 1, 2, 4, 8, 16, 32, 64, 128

CUS = (8, 64, 104, 256, 304)
MAXXB = (1, 55, 56, 57, 111, 112, 113, 255, 256, 257, 641, 1457)
BS = (1, 7, 8, 9, 16, 17, 32, 33, 96, 97, 128, 512)
MS = (1, 8, 128, 129)
SOLVERS = (0, 1)                     # knot / PCR, banded LU
KNOT_THREADS = (64, 128)
MODES = (0, 1, 2)
TAKE = (0, 1, 2)                     # a plan from its start; a take-over of every candidate, its history in place; one of every second candidate, its history ...
PIECES = {64: (64, 1), 128: (33, 4)}  # knot_threads -> (maxN, pieces per wave-task): 64 and 9 wave-tasks
# every knob unset (as ResidentKnobs holds an unset variable) and at one forcing value, one at a time: e, g, clusters_set, clusters, queue, queue_max
UNSET = (0, 0, 0, 0, -1, 3)
KNOBS = (UNSET, (56, 0, 0, 0, -1, 3), (0, 20, 0, 0, -1, 3), (0, 0, 1, 2, -1, 3), (0, 0, 0, 0, 0, 3), (0, 0, 0, 0, 1, 3), (0, 0, 0, 0, -1, 1))


@pytest.fixture(scope="module")
def hc():
    H = _load_hostcheck()
    H.hostcheck_resident_plan_rows.restype = None
    H.hostcheck_resident_plan_rows.argtypes = [C.c_longlong, np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS"), np.ctypeslib.ndpointer(dtype=np.int64, flags="C_CONTIGUOUS")]
    H.hostcheck_resident_capacity.restype = C.c_int
    H.hostcheck_resident_capacity.argtypes = [C.c_int, C.c_int]
    H.hostcheck_round_command_word.restype = C.c_ulonglong
    H.hostcheck_round_command_word.argtypes = [C.c_ulonglong, C.c_int, C.c_int, C.c_int, C.c_double]
    return H


def _grid():
    """Rows of 20 ints in the order hostcheck_resident_plan_rows takes them."""
    ax = np.meshgrid(np.array(SOLVERS), np.array(KNOT_THREADS), np.array(MS), np.array(BS), np.array(MAXXB), np.array(CUS), np.array(MODES),
                     np.array(TAKE), np.arange(len(KNOBS)), indexing="ij")
    solver, kt, m, B, maxXb, cus, mode, take, kn = (a.ravel() for a in ax)
    knobs = np.array(KNOBS)
    maxN, ppw = (np.where(kt == 64, PIECES[64][j], PIECES[128][j]) for j in range(2))
    Bsel = np.where(take == 2, (B + 1) // 2, B)
    have_history = ((take != 2) | (B % 2 == 1)).astype(int)                                    # (... missing at the even batch sizes)
    cols = [solver, kt, m, B, Bsel, maxXb, maxXb, maxN, ppw, cus, mode, (take != 0).astype(int), m, have_history]   # (the shortest vector: maxXb; the history length: m)
    cols += [knobs[kn, j] for j in range(6)]
    return np.ascontiguousarray(np.stack(cols, axis=1).astype(np.int32))


def _parent_plan(r):
    """The driver's lines from its first `return 1` to n_words, vectorised over the rows; why: 0 = applicable, else which `return 1` was taken (1 solver / m / no
    candidate, 2 take-over preconditions, 3 fewer variables than twice the history, 5 no cluster fits, 6 a take-over needs one cluster per straggler, 7 no queue permit)."""
    r = np.ascontiguousarray(r.T)                           # (int32 throughout: the largest figure, n_words at 512 clusters, is below 2^17)
    r = r.T
    solver, kt, m, B, Bsel, min_n, maxXb, maxN, ppw, cus, mode = (r[:, j] for j in range(11))
    take, dv_mem, hist = r[:, 11] != 0, r[:, 12], r[:, 13] != 0
    kE, kG, kCset, kC, kQ, kQmax = r[:, 14], r[:, 15], r[:, 16] != 0, r[:, 17], r[:, 18], r[:, 19]
    why = np.zeros(len(r), np.int64)

    def ret(mask, code):
        why[(why == 0) & mask] = code

    ret((solver != 0) | (m < 1) | (m > 128) | (Bsel < 1), 1)
    ret(take & ((kt != 64) | (m != 128) | (dv_mem != m) | ~hist), 2)
    ret(min_n < 2 * m, 3)
    Es = ROUND_E_SMALL
    Gs = 2 + np.maximum(1, (maxXb + 2 * Es - 1) // (2 * Es))
    E = np.where(~(kE == ROUND_E) & (Gs <= 16) & (8 * Gs * ((Bsel + 7) // 8) <= cus), Es, ROUND_E)
    G = 2 + np.maximum(1, (maxXb + 2 * E - 1) // (2 * E))
    G_min = np.maximum(G, 3)
    tasks = (maxN + ppw - 1) // ppw
    want = np.minimum.reduce([(tasks + 3) // 4 + 2, np.full_like(tasks, 18), cus // np.maximum(Bsel, 1), cus // (8 * ((Bsel + 7) // 8))])
    G = np.maximum(G, want)
    G = np.maximum(G, kG)                                   # (an unset FRX_RESIDENT_G is held as 0)
    G = np.maximum(G, 3)
    S = Bsel.copy()
    over = 8 * G * ((Bsel + 7) // 8) > cus
    G = np.where(over, G_min, G)
    S = np.where(over, np.minimum(Bsel, 8 * (cus // (8 * G))), S)
    by_capacity = over & (S < Bsel)
    ce = ~take & kCset
    by_clusters = ce & (np.maximum(1, kC) < S)
    S = np.where(ce, np.minimum(S, np.maximum(1, kC)), S)
    ret(S < 1, 5)
    ret(take & (S < Bsel), 6)
    queue = (S < B) & ~take
    allowed = np.where(kQ >= 0, kQ != 0, ce | (mode == 2) | (B <= kQmax * S))
    ret(queue & ~allowed, 7)
    NXP = (G - 2) * 2 * E
    n_words = WORDS_PER_CAND * S + 2 + S * G + 4 * B
    ok = why == 0
    out = np.stack([ok, E, G, S, NXP, n_words, queue], axis=1).astype(np.int64)
    out[~ok] = 0
    return out, why, by_capacity & ok, by_clusters & ok


def test_the_plan_over_the_grid(hc):
    rows = _grid()
    assert len(rows) == len(SOLVERS) * len(KNOT_THREADS) * len(MS) * len(BS) * len(MAXXB) * len(CUS) * len(MODES) * len(TAKE) * len(KNOBS)
    got = np.zeros((len(rows), 7), np.int64)
    hc.hostcheck_resident_plan_rows(len(rows), rows, got)
    want, why, by_capacity, by_clusters = _parent_plan(rows)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert len(bad) == 0, f"{len(bad)} rows differ, the first: {rows[bad[0]].tolist()} -> {got[bad[0]].tolist()}, the driver gave {want[bad[0]].tolist()} (return {why[bad[0]]})"
    # the grid reaches every `return 1` and every way S comes out - a thinned grid fails here
    assert set(np.unique(why).tolist()) == {0, 1, 2, 3, 5, 6, 7}
    ok = why == 0
    B, Bsel, S = rows[:, 3], rows[:, 4], want[:, 3]
    assert (ok & (S == Bsel) & (Bsel == B)).any() and by_capacity.any() and by_clusters.any()
    assert (ok & by_capacity & (S < B) & (want[:, 6] == 1)).any() and (ok & by_clusters & (S < B)).any()
    assert set(np.unique(want[ok, 1]).tolist()) == {ROUND_E_SMALL, ROUND_E} and want[ok, 2].max() >= 18 and (want[ok, 2] == 3).any()


def test_the_take_over_capacity(hc):
    """frx_optimize's hand-over threshold: the clusters the chip holds at the large chunk size - and what a plan over more candidates than that comes out with."""
    for cus, maxXb in itertools.product(CUS, MAXXB):
        G = max(3, 2 + max(1, (maxXb + 2 * ROUND_E - 1) // (2 * ROUND_E)))
        assert hc.hostcheck_resident_capacity(maxXb, cus) == 8 * (cus // (8 * G)), (cus, maxXb)
    rows = np.array([[0, 64, 128, 512, 512, 2000, maxXb, 64, 1, cus, 2, 0, 0, 0, 0, 0, 0, 0, -1, 3] for cus, maxXb in itertools.product(CUS, MAXXB)], np.int32)
    got = np.zeros((len(rows), 7), np.int64)
    hc.hostcheck_resident_plan_rows(len(rows), rows, got)
    for r, g in zip(rows, got):
        cap = hc.hostcheck_resident_capacity(int(r[6]), int(r[9]))
        assert (g[0] == 0 and cap == 0) or (g[0] == 1 and g[3] == cap), (r.tolist(), g.tolist(), cap)


def _step_hash(step):
    b = struct.unpack("<Q", struct.pack("<d", step))[0]
    return (b ^ (b >> 24) ^ (b >> 48)) & 0xFFFFFF


def _fields(w):
    """What the kernel extracts from a command word: flags, slot, pair count, sequence number."""
    return w & 0xFF, (w >> 8) & 0xFFF, (w >> 20) & 0xFFF, w >> 32


def test_the_command_word(hc):
    word = hc.hostcheck_round_command_word
    first = DV_EVAL | DV_ADVANCE | DV_TRIAL
    # slot and pair count at both ends of their 12 bits, sequence numbers up to 32 bits
    for seq, slot, bound in itertools.product((1, 2, 0xFFFFFFFF), (0, 0xFFF), (0, 0xFFF)):
        assert _fields(word(seq, first, slot, bound, 0.5)) == (first, slot, bound, seq)
        assert _fields(word(seq, first, slot, bound, 1.0)) == (first | DV_STEP_IS_ONE, slot, bound, seq)     # step exactly 1: the leader confirms from the word alone
    assert _fields(word(7, DV_EVAL, 0, 0, 0.0)) == (DV_EVAL, 0, 0, 7)
    h1 = _step_hash(1.0)                                     # (the first trial of a plan: TRIAL without ADVANCE, so the fold rides here too)
    assert _fields(word(7, DV_EVAL | DV_INIT | DV_TRIAL, 0, 0, 1.0)) == (DV_EVAL | DV_INIT | DV_TRIAL | DV_STEP_IS_ONE, h1 & 0xFFF, h1 >> 12, 7)
    assert _fields(word(7, DV_RESTORE, 0, 0, 0.0)) == (DV_RESTORE, 0, 0, 7)
    # DV_QUIT and DV_NEXT never carry DV_STEP_IS_ONE, whatever the step word says; DV_NEXT's candidate rides in slot | bound << 12
    for step in (0.0, 1.0):
        assert _fields(word(9, DV_QUIT, 0, 0, step)) == (DV_QUIT, 0, 0, 9)
        assert _fields(word(9, DV_NEXT, 4097 & 0xFFF, 4097 >> 12, step)) == (DV_NEXT, 1, 1, 9)
    # a trial inside a search: slot and pair count carry the fold of the step's bits
    for step in (1.0, 0.5, 0.3, 1e-20, 7.25e11, float(np.nextafter(1.0, 2.0))):
        h = _step_hash(step)
        flags = DV_EVAL | DV_TRIAL | (DV_STEP_IS_ONE if step == 1.0 else 0)
        assert _fields(word(3, DV_EVAL | DV_TRIAL, 0xABC, 0x123, step)) == (flags, h & 0xFFF, h >> 12, 3), step
    assert _step_hash(1.0) != _step_hash(float(np.nextafter(1.0, 2.0)))
