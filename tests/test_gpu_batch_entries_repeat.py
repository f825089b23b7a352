"""The five blocking entries that take no handle (fast-racing_amd/csrc/frx_batch.cpp), each called three times in one process on a tiny scene, every output
compared as raw bytes: a device buffer freed early or twice, or one that leaked into the next call, would show here.  The corridor and enumeration entries are
also called once with the capacity one below the need: the refusal leaves the counts as include/frx.h documents, and the call after it succeeds with the same
bytes.  What the entries compute is pinned by the test files of each of them; here only that a call leaves the next one alone."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ERR_CAPACITY = -5
SENTINEL, ISENT = -7.0, -77


def box(lo, hi):
    """the six half-spaces (outward normal, a point of the plane) of an axis-aligned box"""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    rec = []
    for a in range(3):
        for sign, at in ((1.0, hi), (-1.0, lo)):
            n = np.zeros(3); n[a] = sign
            p = (lo + hi) / 2; p[a] = at[a]
            rec.append(np.concatenate([n, p]))
    return np.array(rec)


def same_bytes(runs):
    first = [np.ascontiguousarray(x).tobytes() for x in runs[0]]
    return all([np.ascontiguousarray(x).tobytes() for x in r] == first for r in runs[1:])


def test_enumerate_vertices_batch(frx):
    """two candidates, coarse_n = [1, 2], of boxes: four tasks (a cell; a cell, the overlap, a cell) of eight vertices each"""
    coarse_n = np.array([1, 2], np.int32)
    polys = [box((0, 0, 0), (1, 1, 1)), box((0, 0, 0), (2, 1, 1)), box((1, -0.5, -0.5), (3, 1.5, 1.5))]
    h_off = np.array([0, 6, 12, 18], np.int32); h_rec = np.concatenate(polys).reshape(-1)

    def call(cap_vert):
        status = np.full(4, ISENT, np.int32); v_off = np.full(5, ISENT, np.int32); n_vert = C.c_int(ISENT); v_rec = np.full(3 * 32, SENTINEL)
        rc = frx.lib().frx_enumerate_vertices_batch(0, 2, coarse_n.ctypes.data, h_off.ctypes.data, h_rec.ctypes.data, 16, status.ctypes.data, v_off.ctypes.data,
                                                    cap_vert, C.byref(n_vert), v_rec.ctypes.data)
        return rc, (status, v_off, np.array([n_vert.value]), v_rec)

    runs = [call(32) for _ in range(3)]
    assert [rc for rc, _ in runs] == [0, 0, 0] and same_bytes([out for _, out in runs])
    status, v_off, n_vert, v_rec = runs[0][1]
    assert status.tolist() == [0, 0, 0, 0] and v_off.tolist() == [0, 8, 16, 24, 32] and n_vert[0] == 32 and not (v_rec == SENTINEL).any()
    overlap = v_rec.reshape(-1, 3)[16:24]
    assert overlap.min(axis=0).tolist() == [1.0, 0.0, 0.0] and overlap.max(axis=0).tolist() == [2.0, 1.0, 1.0]
    rc, (status, v_off, n_vert, v_rec) = call(31)                            # one below the need: statuses, offsets and the need are there, no vertex is
    assert rc == ERR_CAPACITY and b"32 vertices, cap_vert is 31" in frx.lib().frx_last_error()
    assert status.tolist() == [0, 0, 0, 0] and v_off.tolist() == [0, 8, 16, 24, 32] and n_vert[0] == 32 and (v_rec == SENTINEL).all()
    rc, out = call(32)
    assert rc == 0 and same_bytes([runs[0][1], out])


@pytest.mark.parametrize("with_map", [True, False], ids=["map", "free"])
def test_corridor_generate_batch(frx, with_map):
    """two paths of 2 and 3 points in a cloud of eight, with and without a 2 x 2 x 2 map whose one occupied cell is off both paths"""
    path_off = np.array([0, 2, 5], np.int32)
    path = np.array([[0.0, 0.0, 1.0], [2.0, 0.0, 1.0], [0.0, 3.0, 1.0], [3.0, 3.0, 1.5], [6.0, 3.0, 1.0]]).reshape(-1)
    obs = np.array([[1.0, 1.2, 1.0], [1.0, -1.1, 1.2], [3.0, 4.1, 1.0], [3.1, 1.9, 0.8], [-0.9, 0.2, 1.0], [5.2, 3.1, 1.1], [1.0, 0.1, 2.4], [2.2, 3.0, 0.2]]).reshape(-1)
    bbox = np.array([2.0, 2.0, 1.5])
    cells = np.zeros(8, np.int8); cells[7] = 100
    vm = frx.VoxelMap([-4.0, -4.0, -1.0], (2, 2, 2), 8.0, cells) if with_map else None
    cap_polys, cap_planes = 4, 32

    def call(cap_rec, room):
        n_polys = np.full(2, ISENT, np.int32); status = np.full(2, ISENT, np.int32); n_rec = C.c_int(ISENT)
        h_off = np.full(2 * cap_polys + 1, ISENT, np.int32); h_rec = np.full(6 * room, SENTINEL)
        rc = frx.lib().frx_corridor_generate_batch(0, 2, path_off.ctypes.data, path.ctypes.data, 8, obs.ctypes.data, bbox.ctypes.data, 3.0, 4.0,
                                                   C.cast(C.pointer(vm._s), C.c_void_p) if vm is not None else None, cap_polys, cap_planes, n_polys.ctypes.data,
                                                   status.ctypes.data, cap_rec, C.byref(n_rec), h_off.ctypes.data, h_rec.ctypes.data)
        return rc, (n_polys, status, np.array([n_rec.value]), h_off, h_rec)

    rc, (n_polys, status, n_rec, h_off, _) = call(2 * cap_polys * cap_planes, 2 * cap_polys * cap_planes)
    assert rc == 0 and status.tolist() == [0, 0] and n_polys.tolist() == [1, 2]              # the second path is longer than max_seg
    need = int(n_rec[0])
    assert need == h_off[3] > h_off[2] > h_off[1] > h_off[0] == 0 and (h_off[4:] == ISENT).all()
    runs = [call(need, need + 4) for _ in range(3)]                          # the capacity equal to the need, four sentinel records behind it
    assert [rc for rc, _ in runs] == [0, 0, 0] and same_bytes([out for _, out in runs])
    h_rec = runs[0][1][4]
    assert not (h_rec[:6 * need] == SENTINEL).any() and (h_rec[6 * need:] == SENTINEL).all()
    assert np.array_equal(runs[0][1][3], h_off) and np.array_equal(runs[0][1][0], n_polys)
    rc, (n_polys1, status1, n_rec1, h_off1, h_rec1) = call(need - 1, need + 4)    # one below: n_polys, status and the need are there, no record is
    assert rc == ERR_CAPACITY and f"{need} records, cap_rec is {need - 1}".encode() in frx.lib().frx_last_error()
    assert np.array_equal(n_polys1, n_polys) and status1.tolist() == [0, 0] and n_rec1[0] == need and (h_rec1 == SENTINEL).all()
    rc, out = call(need, need + 4)
    assert rc == 0 and same_bytes([runs[0][1], out])


@pytest.mark.parametrize("n_obs", [3, 0])
def test_dilate_batch(frx, n_obs):
    """one segment, against three points and against an empty cloud.  The call copies its whole record buffer back and only the first n_planes rows of it are
    defined (include/frx.h), so those rows are what is compared"""
    p1 = np.array([0.0, 0.0, 1.0]); p2 = np.array([2.0, 0.0, 1.0]); bbox = np.array([2.0, 2.0, 1.0])
    obs = np.array([[1.0, 0.8, 1.0], [0.5, -0.9, 1.3], [1.5, 0.2, 1.7]])[:n_obs].reshape(-1)
    cap_planes = 16

    def call():
        npl = np.full(1, ISENT, np.int32); rec = np.full(cap_planes * 6, SENTINEL); Cm = np.full(9, SENTINEL); d = np.full(3, SENTINEL)
        rc = frx.lib().frx_dilate_batch(0, 1, p1, p2, bbox, n_obs, obs.ctypes.data if n_obs else None, 0.0, cap_planes, npl, rec, Cm, d)
        return rc, (npl, rec[:6 * max(int(npl[0]), 0)], Cm, d)

    runs = [call() for _ in range(3)]
    assert [rc for rc, _ in runs] == [0, 0, 0] and same_bytes([out for _, out in runs])
    npl, rec, Cm, d = runs[0][1]
    assert 6 <= npl[0] <= 6 + n_obs and not (rec == SENTINEL).any() and not (Cm == SENTINEL).any() and np.array_equal(d, [1.0, 0.0, 1.0])


def test_map_esdf_on_device(frx):
    """a 3 x 2 x 2 map with one site, only `all` requested"""
    cells = np.zeros(12, np.int8); cells[4] = 100                           # x = 1, y = 1, z = 0
    vm = frx.VoxelMap([0.0, 0.0, 0.0], (3, 2, 2), 0.5, cells)
    runs = [(vm.esdf_on_device(("all",))["all"],) for _ in range(3)]
    assert same_bytes(runs)
    assert np.array_equal(runs[0][0], vm.esdf(("all",))["all"])             # ... and they are the host's bytes, as tests/test_gpu_esdf.py has it for every state


def test_debug_map_blocked_device(frx):
    """two pairs in a 3 x 2 x 2 map with one occupied cell: a line through it and a line above it"""
    cells = np.zeros(12, np.int8); cells[4] = 100                           # x = 1, y = 1, z = 0
    vm = frx.VoxelMap([0.0, 0.0, 0.0], (3, 2, 2), 1.0, cells)
    a = np.array([[0.5, 1.5, 0.5], [0.5, 1.5, 1.5]]); b = np.array([[2.5, 1.5, 0.5], [2.5, 1.5, 1.5]])
    runs = [(vm.is_blocked_device(a, b),) for _ in range(3)]
    assert same_bytes(runs)
    assert runs[0][0].tolist() == [vm.is_blocked(a[0], b[0]), vm.is_blocked(a[1], b[1])] == [True, False]
