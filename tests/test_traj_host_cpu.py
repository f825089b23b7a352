"""What the trajectory entries decide on the host (fast-racing_amd/csrc/frx_traj_host.hpp), in its host build (tests/hostcheck): the entries of frx_traj.cpp
call these functions, so what is pinned here is how a cloud is split, what an offsets array is refused for and with which words, which scalars pass, and
where each part of a scratch buffer begins.  cloud_split is checked against a restatement written here from the two functions it replaced
(clear_geometry and clear_exact_geometry of frx_device.hpp, as they stood), everything else against Python integers and the texts of today.  No GPU."""
import ctypes as C
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_hostcheck import _load_hostcheck  # noqa: E402

OK, INVALID_ARG = 0, -1
INT_MAX = 2 ** 31 - 1
CHECK_MAX_INTERVALS, CLEAR_MAX_POINTS, SAMPLE_FIELDS, GATE_FIELDS = 16384, 1 << 24, 20, 10     # include/frx.h
# the constants of the two old functions: CLEAR_PASS, CLEAR_TARGET_WGS / CLEAR_EXACT_CHUNK, CLEAR_EXACT_TARGET_WGS
DENSE, EXACT = (1024, 2048), (1024, 1024)


@pytest.fixture(scope="module")
def hc():
    H = _load_hostcheck()
    ip = np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS")
    ull = C.c_ulonglong
    H.hostcheck_batch_last_error.restype = C.c_char_p
    H.hostcheck_cloud_constants.restype = None
    H.hostcheck_cloud_constants.argtypes = [ip]
    H.hostcheck_cloud_split.restype = C.c_int
    H.hostcheck_cloud_split.argtypes = [C.c_int] * 5 + [ip]
    H.hostcheck_offsets_args.restype = C.c_int
    H.hostcheck_offsets_args.argtypes = [C.c_char_p, C.c_int, ip, C.c_int]
    H.hostcheck_intervals_arg.restype = C.c_int
    H.hostcheck_intervals_arg.argtypes = [C.c_int]
    H.hostcheck_cloud_points_arg.restype = C.c_int
    H.hostcheck_cloud_points_arg.argtypes = [C.c_int]
    H.hostcheck_sample_time_args.restype = C.c_int
    H.hostcheck_sample_time_args.argtypes = [C.c_int, C.c_double, C.c_double, C.c_int]
    H.hostcheck_sample_rows_arg.restype = C.c_int
    H.hostcheck_sample_rows_arg.argtypes = [C.c_int, C.c_int, C.POINTER(ull)]
    H.hostcheck_carve.restype = None
    H.hostcheck_carve.argtypes = [C.c_int, ull, ull, ull, ip, np.ctypeslib.ndpointer(dtype=np.uint64, flags="C_CONTIGUOUS")]
    return H


def why(hc):
    return hc.hostcheck_batch_last_error().decode()


# ---- the split of a cloud ----
def old_geometry(P, n_obs, force, consts):
    """clear_geometry (consts = DENSE) and clear_exact_geometry (EXACT) as frx_device.hpp carried them: None where they returned 0, else (chunk, nchunks)"""
    unit, target = consts
    c = force
    if force <= 0:
        want = target // P if P < target else 1
        c = (n_obs + want - 1) // want
        c = (c + unit - 1) // unit * unit
    nc = (n_obs + c - 1) // c
    if P * nc > 0x7FFFFFFF:
        return None
    return (c if c < n_obs else n_obs, nc)


def cloud_split(hc, P, n_obs, force, consts):
    out = np.array([-5, -6], np.int32)
    ok = hc.hostcheck_cloud_split(P, n_obs, force, consts[0], consts[1], out)
    assert ok in (0, 1)
    if not ok:
        assert out.tolist() == [-5, -6]                                       # a refusal writes nothing
        return None
    return tuple(out.tolist())


def test_the_call_sites_pass_the_old_constants(hc):
    k = np.zeros(4, np.int32)
    hc.hostcheck_cloud_constants(k)
    assert tuple(k[:2]) == DENSE and tuple(k[2:]) == EXACT


SPLIT_P = (1, 2, 1023, 1024, 1025, 2047, 2048, 2049, 100000)
SPLIT_N = (1, 1023, 1024, 1025, 4097, CLEAR_MAX_POINTS)


@pytest.mark.parametrize("consts", [DENSE, EXACT], ids=["dense", "exact"])
def test_cloud_split_is_the_old_functions(hc, consts):
    n_refused = 0
    for P, n_obs in itertools.product(SPLIT_P, SPLIT_N):
        for force in (0, 1, 7, 1024, n_obs, n_obs + 1):
            want = old_geometry(P, n_obs, force, consts)
            assert cloud_split(hc, P, n_obs, force, consts) == want, (P, n_obs, force)
            n_refused += want is None
            if want is not None:                                              # the chunks tile the cloud, the last one shorter at most
                chunk, nchunks = want
                assert 1 <= chunk <= n_obs and chunk * (nchunks - 1) < n_obs <= chunk * nchunks
    assert n_refused >= 1                                                     # 100000 pieces x 2^24 chunks of one point among them


def test_cloud_split_spelled_out(hc):
    """the restatement above is itself pinned where the old comments stated the rule: whole passes towards the target, one chunk when P alone reaches it"""
    assert cloud_split(hc, 1, 4097, 0, DENSE) == (1024, 5)                    # 2048 wanted: 3 points each, rounded up to a pass
    assert cloud_split(hc, 2048, 4097, 0, DENSE) == (4097, 1) and cloud_split(hc, 2047, 4097, 0, DENSE) == (4097, 1)
    assert cloud_split(hc, 1, CLEAR_MAX_POINTS, 0, DENSE) == (8192, 2048) and cloud_split(hc, 1, CLEAR_MAX_POINTS, 0, EXACT) == (16384, 1024)
    assert cloud_split(hc, 1023, CLEAR_MAX_POINTS, 0, DENSE) == (CLEAR_MAX_POINTS // 2, 2) and cloud_split(hc, 1023, CLEAR_MAX_POINTS, 0, EXACT) == (CLEAR_MAX_POINTS, 1)
    assert cloud_split(hc, 3, 10, 7, DENSE) == (7, 2) and cloud_split(hc, 3, 10, 11, EXACT) == (10, 1)


@pytest.mark.parametrize("consts", [DENSE, EXACT], ids=["dense", "exact"])
def test_cloud_split_refuses_what_does_not_fit_a_grid(hc, consts):
    """force = 1 makes a chunk of every point: 128 pieces x 2^24 chunks = 2^31, one more than a grid holds; 127 pieces fit"""
    assert 127 * CLEAR_MAX_POINTS <= INT_MAX < 128 * CLEAR_MAX_POINTS
    assert old_geometry(128, CLEAR_MAX_POINTS, 1, consts) is None and cloud_split(hc, 128, CLEAR_MAX_POINTS, 1, consts) is None
    assert cloud_split(hc, 127, CLEAR_MAX_POINTS, 1, consts) == old_geometry(127, CLEAR_MAX_POINTS, 1, consts) == (1, CLEAR_MAX_POINTS)
    assert cloud_split(hc, INT_MAX, 2, 1, consts) is None and cloud_split(hc, INT_MAX, 2, 0, consts) == (2, 1)   # no overflow on the way to the verdict


# ---- the offsets rule ----
WHO = ("frx_contain_fold: piece_off", "frx_clearance_exact_fold: piece_off", "frx_map_distance_fold: piece_off", "gate_off")


def offsets(hc, what, off, from_zero):
    off = np.ascontiguousarray(off, dtype=np.int32)
    rc = hc.hostcheck_offsets_args(what.encode(), len(off) - 1, off, int(from_zero))
    return rc, why(hc)


@pytest.mark.parametrize("what", WHO)
def test_offsets_rule_refusal_by_refusal(hc, what):
    from_zero = what == "gate_off"                                            # the gates' offsets start at 0, a fold's piece_off anywhere from 0 on
    assert offsets(hc, what, [0, 2, 2, 5], from_zero) == (OK, "")
    assert offsets(hc, what, [0, 0], from_zero) == (OK, "")
    assert offsets(hc, what, [-1, 2, 3], from_zero) == (INVALID_ARG, what + ("[0] must be 0" if from_zero else "[0] must be >= 0"))
    assert offsets(hc, what, [3, 3, 4], from_zero) == ((INVALID_ARG, what + "[0] must be 0") if from_zero else (OK, ""))
    assert offsets(hc, what, [0, 2, 1, 5], from_zero) == (INVALID_ARG, what + " must not fall (candidate 1)")
    assert offsets(hc, what, [0, -1], from_zero) == (INVALID_ARG, what + " must not fall (candidate 0)")
    assert offsets(hc, what, [0, 4, 3, 2], from_zero) == (INVALID_ARG, what + " must not fall (candidate 1)")     # the first fall is the one named
    assert offsets(hc, what, [-2, -3], from_zero)[1].endswith("[0] must be 0" if from_zero else "[0] must be >= 0")   # the start before the walk
    assert offsets(hc, what, [0, 1], from_zero) == (OK, "")                   # and a success clears the text


def test_offsets_texts_are_the_entries(frx):
    """the same words through the library's own entries, which need no device for them"""
    L = frx.lib()
    d = np.zeros(64); dp = d.ctypes.data
    up = np.array([1, 2, 3], np.int32); low = np.array([-1, 2, 3], np.int32); fall = np.array([0, 2, 1], np.int32)
    for name, extra in (("frx_contain_fold", ()), ("frx_clearance_exact_fold", ()), ("frx_map_distance_fold", (0.0,))):
        fn = getattr(L, name)
        assert fn(2, low.ctypes.data, dp, dp, *extra, dp, None) == INVALID_ARG and L.frx_last_error().decode() == name + ": piece_off[0] must be >= 0"
        assert fn(2, fall.ctypes.data, dp, dp, *extra, dp, None) == INVALID_ARG and L.frx_last_error().decode() == name + ": piece_off must not fall (candidate 1)"
    fl = np.zeros(2, np.uint32)
    assert L.frx_gate_flags(2, up.ctypes.data, dp, fl.ctypes.data) == INVALID_ARG and L.frx_last_error().decode() == "gate_off[0] must be 0"
    assert L.frx_gate_flags(2, fall.ctypes.data, dp, fl.ctypes.data) == INVALID_ARG and L.frx_last_error().decode() == "gate_off must not fall (candidate 1)"


# ---- the scalars ----
def test_intervals_and_cloud_points(hc):
    for n in (1, 2, 256, CHECK_MAX_INTERVALS):
        assert hc.hostcheck_intervals_arg(n) == OK and why(hc) == ""
    for n in (0, -1, CHECK_MAX_INTERVALS + 1, INT_MAX, -INT_MAX - 1):
        assert hc.hostcheck_intervals_arg(n) == INVALID_ARG and why(hc) == "intervals must lie in 1..16384"
    for n in (1, 5, CLEAR_MAX_POINTS):
        assert hc.hostcheck_cloud_points_arg(n) == OK and why(hc) == ""
    for n in (0, -4, CLEAR_MAX_POINTS + 1, INT_MAX):
        assert hc.hostcheck_cloud_points_arg(n) == INVALID_ARG and why(hc) == "n_obs must lie in 1..16777216"


def test_sample_rules_case_by_case(hc):
    """the cases of tests/test_trajectory_sample_cpu.py::test_invalid_arguments, each with the code and the words it looks for"""
    inf, nan = float("inf"), float("nan")
    for S in (0, -1):
        assert hc.hostcheck_sample_time_args(S, 0.0, 0.01, 0) == INVALID_ARG and "n_samples" in why(hc)
        assert hc.hostcheck_sample_time_args(S, 0.0, 0.0, 1) == INVALID_ARG and why(hc) == "n_samples must be >= 1"
    assert hc.hostcheck_sample_time_args(1, 0.0, 0.0, 0) == INVALID_ARG and "dt == 0" in why(hc)                 # spread over the duration: S >= 2
    assert hc.hostcheck_sample_time_args(1, 0.0, 0.0, 1) == OK and hc.hostcheck_sample_time_args(1, 0.0, 0.01, 0) == OK   # ... not with times or a step
    assert hc.hostcheck_sample_time_args(2, 0.0, 0.0, 0) == OK and why(hc) == ""
    for t0, dt in ((0.0, -0.01), (0.0, -inf), (0.0, nan), (0.0, inf), (nan, 0.01), (inf, 0.0), (-inf, 0.01)):
        for have_times in (0, 1):
            assert hc.hostcheck_sample_time_args(8, t0, dt, have_times) == INVALID_ARG and why(hc) == "t0 and dt must be finite and dt >= 0", (t0, dt)
    assert hc.hostcheck_sample_time_args(8, -3.5, 0.0, 0) == OK
    # the count of doubles: B x S x 20 as a size_t, refused where it overflows and written only where it does not
    n = C.c_ulonglong(77)
    assert hc.hostcheck_sample_rows_arg(3, 7, C.byref(n)) == OK and n.value == 3 * 7 * SAMPLE_FIELDS
    assert C.sizeof(C.c_size_t) == 8
    assert hc.hostcheck_sample_rows_arg(INT_MAX, 1 << 28, C.byref(n)) == OK and n.value == INT_MAX * (1 << 28) * SAMPLE_FIELDS < 2 ** 64
    n = C.c_ulonglong(77)
    assert INT_MAX * INT_MAX < 2 ** 64 <= INT_MAX * INT_MAX * SAMPLE_FIELDS   # the product of the two counts fits, its rows do not
    assert hc.hostcheck_sample_rows_arg(INT_MAX, INT_MAX, C.byref(n)) == INVALID_ARG and why(hc) == "n_samples x B x FRX_SAMPLE_FIELDS overflows size_t" and n.value == 77


# ---- the carve-ups ----
def carve(hc, kind, a, b=0, c=0, dim=(1, 1, 1)):
    out = np.zeros(3, np.uint64)
    hc.hostcheck_carve(kind, a, b, c, np.array(dim, np.int32), out)
    return tuple(int(v) for v in out)


def test_carve_ups_against_python_integers(hc):
    for P, n_obs, nchunks in ((1, 1, 1), (10, 5, 1), (10, 4097, 5), (100000, CLEAR_MAX_POINTS, 2048), (INT_MAX, CLEAR_MAX_POINTS, 1)):
        for fields, n_work in ((4, 4 * P * nchunks if nchunks > 1 else 0), (6, 10 * P * nchunks)):   # the dense and the exact clearance in d_clear
            n_rows = fields * P
            assert carve(hc, 0, n_rows, n_obs, n_work) == (n_rows, n_rows + 3 * n_obs, n_rows + 3 * n_obs + n_work)
    for n_gates, B in ((1, 1), (3, 3), (7, 2), (1 << 20, 1 << 16), (INT_MAX, INT_MAX)):
        second, third, total = carve(hc, 1, n_gates, B)
        assert (second, third) == (GATE_FIELDS * n_gates, (GATE_FIELDS + 9) * n_gates)
        assert total == third + (B + 2) // 2 and 8 * (total - third) >= 4 * (B + 1) > 8 * (total - third - 1)    # B + 1 ints in whole doubles, none to spare
    for n_out in (0, 20, 20 * 3 * 7, 20 * (1 << 40)):
        assert carve(hc, 2, n_out, 0) == (n_out, n_out, n_out)
        assert carve(hc, 2, n_out, 1) == (n_out, n_out + n_out // SAMPLE_FIELDS, n_out + n_out // SAMPLE_FIELDS)
        assert (8 * n_out) % 16 == 0                                          # the rows come first: 16-byte aligned for any count
    for n_rows, dim in ((4, (1, 1, 1)), (40, (8, 8, 8)), (4 * 100000, (1290, 1290, 1290)), (12, (INT_MAX, 1, 1))):
        cells = dim[0] * dim[1] * dim[2]
        assert carve(hc, 3, n_rows, dim=dim) == (n_rows, n_rows + cells, n_rows + cells)
