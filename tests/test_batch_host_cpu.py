"""What the handle-less batch entries decide on the host (fast-racing_amd/csrc/frx_batch_host.hpp), in its host build (tests/hostcheck): the entries of
frx_batch.cpp call these functions, so what is pinned here is what the device is sent and what the caller gets back.  The task list of the vertex enumeration is
checked against a restatement written here from include/frx.h's description of the order (cell 0, overlap 0|1, cell 1, ...), pack_slots against a Python
concatenation, the need against Python integers, the voxel map's rule refusal by refusal.  No GPU."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_hostcheck import _load_hostcheck  # noqa: E402

OK, INVALID_ARG = 0, -1
INT_MAX = 2 ** 31 - 1
SENTINEL, ISENT = -7.0, -77


@pytest.fixture(scope="module")
def hc():
    H = _load_hostcheck()
    ip = np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS")
    dp = np.ctypeslib.ndpointer(dtype=np.float64, flags="C_CONTIGUOUS")
    H.hostcheck_batch_last_error.restype = C.c_char_p
    H.hostcheck_enum_tasks.restype = C.c_longlong
    H.hostcheck_enum_tasks.argtypes = [C.c_int, ip, ip, ip, C.c_longlong]
    H.hostcheck_pack_slots.restype = C.c_int
    H.hostcheck_pack_slots.argtypes = [C.c_int, C.c_int, ip, C.c_longlong, dp, C.c_int, dp, ip]
    H.hostcheck_need_fits.restype = C.c_int
    H.hostcheck_need_fits.argtypes = [C.c_int, ip, C.c_int, C.POINTER(C.c_longlong), C.POINTER(C.c_int)]
    H.hostcheck_voxel_map_args.restype = C.c_int
    H.hostcheck_voxel_map_args.argtypes = [ip, C.c_double, C.c_void_p, C.c_int]
    return H


# ---- the task list ----
def tasks_restated(coarse_n, h_off):
    """[n][4] of (first record, planes, second range's first record, its planes): a cell is one range, an overlap the ranges of both cells; a task whose first
    range is empty takes the second as its only one, and one without planes at all carries -1"""
    out, m = [], 0
    for n in coarse_n:
        for i in range(n):
            ranges = [[(h_off[m + i], h_off[m + i + 1] - h_off[m + i])]]
            if i + 1 < n:
                ranges.append(ranges[0] + [(h_off[m + i + 1], h_off[m + i + 2] - h_off[m + i + 1])])
            for r in ranges:
                r = r + [(0, 0)] * (2 - len(r))
                if r[0][1] == 0:
                    r = [(r[0][0], r[1][1]), (0, 0)]
                out.append([r[0][0], r[0][1] if r[0][1] else -1, r[1][0], r[1][1]])
        m += n
    return np.array(out, np.int32).reshape(-1, 4)


def enum_tasks(hc, coarse_n, h_off):
    coarse_n = np.ascontiguousarray(coarse_n, dtype=np.int32); h_off = np.ascontiguousarray(h_off, dtype=np.int32)
    cap = min(int(2 * np.maximum(coarse_n, 0).sum()) + 1, 1024)
    tasks = np.full(4 * cap, ISENT, np.int32)
    n = hc.hostcheck_enum_tasks(len(coarse_n), coarse_n, h_off, tasks, cap)
    return n, tasks[:4 * max(n, 0)].reshape(-1, 4), tasks[4 * max(n, 0):], hc.hostcheck_batch_last_error().decode()


TASK_CASES = {
    "one_cell": ([1], [0, 6]),
    "one_and_three": ([1, 3], [0, 6, 14, 20, 29]),
    "empty_in_front": ([2], [0, 0, 7]),                                       # the overlap takes the second range as its only one
    "empty_behind": ([2], [0, 7, 7]),
    "two_empty_neighbours": ([3], [0, 5, 5, 5]),                              # K = -1 for both empty cells and their overlap
    "offset_start": ([2, 1], [11, 17, 25, 31]),                               # a non-zero h_off[0]
}


@pytest.mark.parametrize("name", TASK_CASES)
def test_task_list(hc, name):
    coarse_n, h_off = TASK_CASES[name]
    n, tasks, rest, _ = enum_tasks(hc, coarse_n, h_off)
    want = tasks_restated(coarse_n, h_off)
    assert n == len(want) == 2 * sum(coarse_n) - len(coarse_n)
    assert np.array_equal(tasks, want), (tasks.tolist(), want.tolist())
    assert (rest == ISENT).all()


def test_task_list_spelled_out(hc):
    """the restatement above is itself pinned on the cases the entry's comment names"""
    assert enum_tasks(hc, [1], [0, 6])[1].tolist() == [[0, 6, 0, 0]]
    assert enum_tasks(hc, [2], [0, 0, 7])[1].tolist() == [[0, -1, 0, 0], [0, 7, 0, 0], [0, 7, 0, 0]]
    assert enum_tasks(hc, [2], [0, 7, 7])[1].tolist() == [[0, 7, 0, 0], [0, 7, 7, 0], [7, -1, 0, 0]]
    assert enum_tasks(hc, [3], [0, 5, 5, 5])[1].tolist() == [[0, 5, 0, 0], [0, 5, 5, 0], [5, -1, 0, 0], [5, -1, 0, 0], [5, -1, 0, 0]]
    assert enum_tasks(hc, [2, 1], [11, 17, 25, 31])[1].tolist() == [[11, 6, 0, 0], [11, 6, 17, 8], [17, 8, 0, 0], [25, 6, 0, 0]]


def test_task_list_refusals(hc):
    n, _, _, why = enum_tasks(hc, [2, 1, 0, 1], [0, 1, 2, 3, 4])
    assert n == INVALID_ARG and "coarse_n[2] < 1" in why
    n, _, _, why = enum_tasks(hc, [1, -3], [0, 1])
    assert n == INVALID_ARG and "coarse_n[1] < 1" in why
    n, _, _, why = enum_tasks(hc, [2, 2], [0, 4, 9, 8, 12])
    assert n == INVALID_ARG and "not monotone at polytope 2" in why
    n, _, _, why = enum_tasks(hc, [1], [-1, 4])
    assert n == INVALID_ARG and "h_off[0] < 0" in why
    # 2 n - B tasks of four ints must stay below 2^31: the count is refused before h_off is walked (two entries are all it has here)
    assert 2 * (2 ** 28 + 1) - 1 > INT_MAX // 4 >= 2 * 2 ** 28 - 1
    n, _, _, why = enum_tasks(hc, [2 ** 28 + 1], [0, 1])
    assert n == INVALID_ARG and "too many polytopes" in why
    n, tasks, _, why = enum_tasks(hc, [1], [0, 4])                           # and a success clears the text
    assert n == 1 and why == ""


# ---- pack_slots ----
def pack(hc, W, groups, room=5):
    """groups: list of (count [n], widest).  Every group is staged at its widest count with values of its own; returns (rec, off, used) after all groups, rec
    with `room` sentinel rows behind the need, next to the Python concatenation"""
    rng = np.random.default_rng(W * 100 + len(groups))
    need = sum(int(np.sum(c)) for c, _ in groups); slots = sum(len(c) for c, _ in groups)
    rec = np.full(W * (need + room), SENTINEL); off = np.full(slots + 1 + room, ISENT, np.int32); off[0] = 0
    want, want_off, used, poly = [], [0], 0, 0
    for count, widest in groups:
        count = np.ascontiguousarray(count, dtype=np.int32)
        stage = rng.uniform(-9.0, 9.0, (len(count), widest, W)) if widest else np.zeros((len(count), 0, W))
        for t, k in enumerate(count):
            want.append(stage[t, :k].reshape(-1)); want_off.append(want_off[-1] + int(k))
        used = hc.hostcheck_pack_slots(W, len(count), count, widest, np.ascontiguousarray(stage.reshape(-1)) if stage.size else np.zeros(1), used, rec, off[poly:])
        poly += len(count)
    want = np.concatenate(want) if want else np.zeros(0)
    assert used == need == want_off[-1]
    assert np.array_equal(rec[:W * need], want) and (rec[W * need:] == SENTINEL).all()          # nothing beyond the need
    assert off[:slots + 1].tolist() == want_off and (off[slots + 1:] == ISENT).all()
    return rec, off, used


@pytest.mark.parametrize("W", [3, 6])
def test_pack_slots(hc, W):
    pack(hc, W, [([0, 3, 0, 0, 2, 5, 0], 5)])                                # zeros between non-zero counts
    pack(hc, W, [([4, 4, 4], 4)])                                            # every count equal to widest
    pack(hc, W, [([7], 7)])                                                  # a single slot
    pack(hc, W, [([1], 1)])
    pack(hc, W, [([2, 0, 3], 3), ([0, 4, 1, 4], 4)])                         # a second group behind a first: the offsets continue
    pack(hc, W, [([2, 1], 2), ([0, 0], 0), ([3], 3)])                        # ... also over a group without rows


@pytest.mark.parametrize("W", [3, 6])
def test_pack_slots_widest_zero(hc, W):
    """widest = 0: no record is written and no staged value read (there is none); the group's offsets repeat what was taken before it, as the CSR of n empty
    polytopes must"""
    rec, off, used = pack(hc, W, [([0, 0, 0], 0)])
    assert used == 0 and (rec == SENTINEL).all() and off[:4].tolist() == [0, 0, 0, 0]


# ---- the need ----
def need_fits(hc, count, cap):
    need, rep = C.c_longlong(), C.c_int()
    ok = hc.hostcheck_need_fits(len(count), np.ascontiguousarray(count, dtype=np.int32), cap, C.byref(need), C.byref(rep))
    return ok, need.value, rep.value


def test_need_is_clipped_in_the_report_and_not_in_the_verdict(hc):
    big = [2 ** 30, 2 ** 30, 2 ** 30]
    for cap in (0, 1, 2 ** 30, INT_MAX):
        assert need_fits(hc, big, cap) == (0, 3 * 2 ** 30, INT_MAX)           # above 2^31 - 1: reported clipped, refused against any int capacity
    assert need_fits(hc, [2 ** 30, 2 ** 30 - 1], INT_MAX) == (1, INT_MAX, INT_MAX)
    assert need_fits(hc, [2 ** 30, 2 ** 30], INT_MAX) == (0, 2 ** 31, INT_MAX)
    assert need_fits(hc, [3, 0, 4], 7) == (1, 7, 7)                           # equal to the capacity: accepted
    assert need_fits(hc, [3, 0, 4], 6) == (0, 7, 7)
    assert need_fits(hc, [3, 0, 4], 8) == (1, 7, 7)
    assert need_fits(hc, [0], 0) == (1, 0, 0)


# ---- the voxel map's rule ----
def map_args(hc, dim, res=0.25, cells=True, need_cells=True):
    never_read = C.c_void_p(64) if cells else None                            # a non-null address that is not memory: the rule reads no cell
    rc = hc.hostcheck_voxel_map_args(np.array(dim, np.int32), res, never_read, int(need_cells))
    return rc, hc.hostcheck_batch_last_error().decode()


@pytest.mark.parametrize("need_cells", [True, False])
def test_voxel_map_rules_one_by_one(hc, need_cells):
    assert map_args(hc, (2, 2, 2), need_cells=need_cells) == (OK, "")
    for res in (0.0, -1.0, float("nan")):
        rc, why = map_args(hc, (2, 2, 2), res=res, need_cells=need_cells)
        assert rc == INVALID_ARG and why.startswith("hostcheck: ") and "res > 0" in why
    for axis in range(3):
        for bad in (0, -4):
            dim = [3, 3, 3]; dim[axis] = bad
            rc, why = map_args(hc, dim, need_cells=need_cells)
            assert rc == INVALID_ARG and "dim > 0 on all three axes" in why
    rc, why = map_args(hc, (2, 2, 2), cells=False, need_cells=need_cells)     # cells only where the entry reads them
    assert (rc, "cells" in why) == ((INVALID_ARG, True) if need_cells else (OK, False))
    assert ("needs cells" in map_args(hc, (0, 2, 2), need_cells=need_cells)[1]) == need_cells


@pytest.mark.parametrize("need_cells", [True, False])
def test_voxel_map_cell_limits(hc, need_cells):
    rc, why = map_args(hc, (46341, 46341, 1), need_cells=need_cells)          # 46341^2 = 2^31 + 4633: one layer is too many
    assert rc == INVALID_ARG and "2^31 - 1" in why
    assert map_args(hc, (46340, 46340, 1), need_cells=need_cells)[0] == OK
    assert map_args(hc, (1, 46341, 46341), need_cells=need_cells)[0] == INVALID_ARG       # ... and so is the whole grid with a small layer
    assert 1290 ** 3 == 2146689000 <= INT_MAX < 1291 ** 3 == 2151685171
    assert map_args(hc, (1290, 1290, 1290), need_cells=need_cells) == (OK, "")
    rc, why = map_args(hc, (1291, 1291, 1291), need_cells=need_cells)
    assert rc == INVALID_ARG and "2^31 - 1" in why
    assert map_args(hc, (INT_MAX, 1, 1), need_cells=need_cells)[0] == OK
    assert map_args(hc, (INT_MAX, INT_MAX, INT_MAX), need_cells=need_cells)[0] == INVALID_ARG   # no overflow on the way to the verdict
