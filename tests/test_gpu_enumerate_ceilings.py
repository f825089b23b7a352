"""k_enumerate (frx_enumerate_kernel.hpp) above 64 planes and 256 vertices, and k_slots_to_tasks alone, against the host's frx_enumerate_vertices with ==.

The workgroup is four waves of 64 lanes.  One lane converts one plane and tests one plane's slack, so everything decided by `t < K` needs K > 64 to reach
waves 1 - 3 and K = 256 to fill them; the order loop takes 256 vertices a trip, so nv > 256 runs its second trip; the accepted list lives in dynamic LDS of
52 cap_v bytes, 26 KB at cap_v = 512.  The states of tests/enumerate_states.py stand on either side of each of these edges (test_enumerate_states_cpu.py
asserts their counts and properties on the host); here each large task stands between small healthy ones whose slots must keep their bits."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import enumerate_reference as er  # noqa: E402
import enumerate_states as es  # noqa: E402
from test_gpu_enumerate_batch import ISENT, PAD, SENTINEL, assert_parity, blocking_polys, device_enum, host_rows, pack  # noqa: E402
from test_gpu_trajectory_sample import DevBuf  # noqa: E402

pytestmark = pytest.mark.gpu

_small = {}


def small_slots(frx, cap_v):
    """cube() and tetrahedron() alone at this cap_v: what they must give as anybody's neighbours"""
    if cap_v not in _small:
        slot, nv, st = device_enum(frx, *pack([es.cube(), es.tetrahedron()]), cap_v)
        assert nv.tolist() == [8, 4] and st.tolist() == [0, 0]
        assert np.array_equal(slot[0, :8], host_rows(frx, es.cube())[1]) and np.array_equal(slot[1, :4], host_rows(frx, es.tetrahedron())[1])
        _small[cap_v] = slot
    return _small[cap_v]


def between(frx, mid, cap_v):
    """cube(), mid, tetrahedron() as one batch; the neighbours' whole slots must be those of the two run alone.  Returns mid's (slot, nv, status)"""
    slot, nv, st = device_enum(frx, *pack([es.cube(), mid, es.tetrahedron()]), cap_v)
    alone = small_slots(frx, cap_v)
    assert st[0] == 0 and st[2] == 0 and nv[0] == 8 and nv[2] == 4 and np.array_equal(slot[0], alone[0]) and np.array_equal(slot[2], alone[1])
    return slot[1], nv[1], st[1]


def assert_host(frx, rec, slot, nv, st):
    hn, hv, hs = host_rows(frx, rec)
    assert nv == hn and st == hs, (nv, hn, st, hs)
    assert np.array_equal(slot[:hn], hv), np.argwhere(slot[:hn] != hv)[:4].tolist()


# ---- plane counts ----
def test_plane_counts_in_one_batch(frx):
    _, nv, _ = assert_parity(frx, [es.sphere(K, 1) for K in es.CEILING_K], cap_v=160, statuses=[0] * 9)
    assert nv.tolist() == list(es.CEILING_NV)


@pytest.mark.parametrize("K", es.CEILING_K)
def test_plane_count_between_neighbours(frx, K):
    rec = es.sphere(K, 1)
    assert_host(frx, rec, *between(frx, rec, 160))


# ---- vertex counts ----
def test_second_trip_of_the_order_loop(frx):
    polys = [es.prism(128), es.prism(129), es.pyramid(254), es.pyramid(255)]
    slot, nv, st = assert_parity(frx, polys, cap_v=264, statuses=[0] * 4)
    assert nv.tolist() == [256, 258, 255, 256]
    rec = es.pyramid(255)                                                   # the apex: C(255, 3) triples of one key, the survivor carries the first one's own bits
    first = er.triple_point(rec, 0, 1, 2)
    keys = np.rint(slot[3, :256] / 1e-7).astype(np.int64)
    at = np.nonzero((keys == np.rint(first / 1e-7).astype(np.int64)).all(axis=1))[0]
    assert len(at) == 1 and np.array_equal(slot[3, at[0]], first)


@pytest.mark.parametrize("name", ["prism128", "prism129", "pyramid254", "pyramid255"])
def test_vertex_count_between_neighbours(frx, name):
    rec = {"prism128": es.prism(128), "prism129": es.prism(129), "pyramid254": es.pyramid(254), "pyramid255": es.pyramid(255)}[name]
    assert_host(frx, rec, *between(frx, rec, 264))


def test_the_largest_accepted_list(frx):
    prism, tangent = es.prism(254), es.sphere(256, 1, spread=0.0)
    polys = [es.cube(), prism, es.tetrahedron(), tangent, es.cube()]
    tasks, rec = pack(polys)
    got = {cap_v: device_enum(frx, tasks, rec, cap_v) for cap_v in (512, 508, 507)}
    for cap_v in (512, 508):                                                # room to spare, and exactly enough
        slot, nv, st = got[cap_v]
        assert st.tolist() == [0] * 5 and nv.tolist() == [8, 508, 4, 508, 8]
        for t, p in enumerate(polys):
            assert_host(frx, p, slot[t], nv[t], st[t])
    slot, nv, st = got[507]                                                 # one short: refused, nothing written (device_enum checked the slot behind nv = 0)
    assert st.tolist() == [0, frx.HV_VERTICES, 0, frx.HV_VERTICES, 0] and nv.tolist() == [8, 0, 4, 0, 8]
    assert (slot[1] == SENTINEL).all() and (slot[3] == SENTINEL).all()
    for t in (0, 2, 4):
        assert np.array_equal(slot[t, :nv[t]], got[508][0][t, :nv[t]])


def test_the_smallest_accepted_list(frx):
    slot, nv, st = device_enum(frx, *pack([es.tetrahedron(), es.cube(), es.tetrahedron()]), cap_v=4)
    assert st.tolist() == [0, frx.HV_VERTICES, 0] and nv.tolist() == [4, 0, 4] and (slot[1] == SENTINEL).all()
    tet = host_rows(frx, es.tetrahedron())[1]
    assert np.array_equal(slot[0], tet) and np.array_equal(slot[2], tet)


# ---- verdicts ----
@pytest.mark.parametrize("name, want, nv_want", [("flat_late", 2, 4), ("open_late", 1, 4), ("open_sides", 1, 0)])
def test_verdicts_decided_beyond_the_first_wave(frx, name, want, nv_want):
    rec = getattr(es, name)()
    hn, hv, hs = host_rows(frx, rec)                                        # the host's count and verdict, the restatement's vertices
    assert (hs, hn) == (want, nv_want) and (frx.HV_UNBOUNDED, frx.HV_FLAT) == (1, 2)
    assert_host(frx, rec, *between(frx, rec, 64))


# ---- refusals decided outside wave 0 ----
@pytest.mark.parametrize("record", [64, 128, 255])
@pytest.mark.parametrize("value", [np.nan, np.inf, -np.inf])
def test_nonfinite_record_beyond_the_first_wave(frx, record, value):
    rec = es.sphere(256, 1).copy()
    rec[record, (record + (0 if np.isnan(value) else 3)) % 6] = value       # a normal component or a point component, by record
    slot, nv, st = between(frx, rec, 160)
    assert st == frx.HV_NONFINITE and nv == 0 and (slot == SENTINEL).all()


# ---- two-range tasks ----
def two_range(rec, c0):
    """(task, record array): the first c0 records of rec stored BEHIND the others, records of NaN in front, between and behind"""
    c1 = len(rec) - c0
    gap = np.full((3, 6), np.nan)
    arr = np.concatenate([gap, rec[c0:], gap, gap, rec[:c0], gap])
    return [3 + c1 + 6, c0, 3, c1], arr


def test_two_ranges_equal_one_range(frx):
    rec = es.sphere(256, 1)
    hn, hv, hs = host_rows(frx, rec)
    one, nv1, st1 = device_enum(frx, *pack([rec]), cap_v=160)
    assert st1[0] == 0 and nv1[0] == hn == 142 and np.array_equal(one[0, :hn], hv)
    for c0 in (1, 128, 255):
        task, arr = two_range(rec, c0)
        assert np.array_equal(np.concatenate([arr[task[0]:task[0] + task[1]], arr[task[2]:task[2] + task[3]]]), rec)
        slot, nv, st = device_enum(frx, [task], arr, cap_v=160)
        assert st[0] == 0 and nv[0] == hn and np.array_equal(slot[0], one[0]), c0
    task, arr = two_range(es.tetrahedron(), 1)
    slot, nv, st = device_enum(frx, [task], arr, cap_v=160)
    assert st[0] == 0 and nv[0] == 4 and np.array_equal(slot[0, :4], host_rows(frx, es.tetrahedron())[1])


def test_two_range_refusals(frx):
    """the counts alone decide: no record is read (every record but the neighbours' is NaN, and a read would say FRX_HV_NONFINITE)"""
    left, right = es.cube(), es.tetrahedron()
    arr = np.concatenate([left, np.full((300, 6), np.nan), right])
    cases = [((128, 129), frx.HV_PLANES), ((2, 1), frx.HV_PLANES), ((1, 2), frx.HV_PLANES), ((-1, 5), frx.HV_PLANES), ((5, -1), frx.HV_PLANES), ((0, 6), frx.HV_SKIPPED)]
    tasks = [[0, 6, 0, 0]]
    for (c0, c1), _ in cases:
        tasks += [[6, c0, 150, c1], [306, 4, 0, 0]]
    slot, nv, st = device_enum(frx, tasks, arr, cap_v=64)
    alone = small_slots(frx, 64)
    assert np.array_equal(slot[0], alone[0]) and st[0] == 0 and nv[0] == 8
    for i, ((c0, c1), want) in enumerate(cases):
        assert st[1 + 2 * i] == want and nv[1 + 2 * i] == 0 and (slot[1 + 2 * i] == SENTINEL).all(), (c0, c1)
        assert st[2 + 2 * i] == 0 and nv[2 + 2 * i] == 4 and np.array_equal(slot[2 + 2 * i], alone[1]), (c0, c1)


# ---- the blocking form ----
def test_blocking_form_cuts_at_the_widest_polytope(frx):
    cells = [[es.cube(), es.tetrahedron()], [es.prism(254)], [es.tetrahedron()]]
    coarse_n = np.array([len(c) for c in cells], np.int32)
    flat = [rec for c in cells for rec in c]
    h_off = np.zeros(len(flat) + 1, np.int32); h_off[1:] = np.cumsum([len(r) for r in flat]); h_rec = np.concatenate(flat)
    v_off, v_rec, status = frx.enumerate_vertices_batch(coarse_n, h_off, h_rec, cap_v=512)
    polys = blocking_polys(coarse_n, h_off, h_rec)
    rows = [host_rows(frx, p) for p in polys]
    assert len(polys) == 5 and [len(p) for p in polys] == [6, 10, 4, 256, 4] and max(r[0] for r in rows) == 508
    assert status.tolist() == [r[2] for r in rows] and status[3] == 0
    assert v_off.tolist() == np.concatenate([[0], np.cumsum([r[0] for r in rows])]).tolist()
    assert np.array_equal(v_rec, np.concatenate([r[1].reshape(-1) for r in rows]))


# ---- k_slots_to_tasks alone ----
def slots_to_tasks_ref(n_paths, cap_polys, cap_planes, cell_planes, n_polys):
    out = np.zeros((n_paths, 2 * cap_polys - 1, 4), np.int64)
    for p, q in np.ndindex(n_paths, 2 * cap_polys - 1):
        cell = p * cap_polys + q // 2
        if q // 2 + q % 2 < n_polys[p]:                                      # a cell that exists, or an overlap whose second cell exists
            out[p, q, :2] = cell * cap_planes, cell_planes[cell]
            if q % 2:
                out[p, q, 2:] = (cell + 1) * cap_planes, cell_planes[cell + 1]
    return out


@pytest.mark.parametrize("n_paths, cap_polys, positions", [(85, 2, 255), (86, 2, 258), (1, 129, 257)])
def test_slots_to_tasks_alone(frx, n_paths, cap_polys, positions):
    cap_planes = 96
    per = 2 * cap_polys - 1
    assert n_paths * per == positions
    rng = np.random.default_rng(positions)
    cell_planes = rng.integers(1, cap_planes + 1, n_paths * cap_polys).astype(np.int32)
    many = rng.integers(0, cap_polys + 1, n_paths).astype(np.int32); many[:3] = [0, 1, cap_polys][:n_paths]
    runs = [many] if n_paths > 1 else [np.array([v], np.int32) for v in (0, 1, 64, cap_polys)]
    for n_polys in runs:
        assert n_paths == 1 or {0, 1, cap_polys} <= set(n_polys.tolist())
        tasks0 = np.full(positions * 4 + PAD, ISENT, np.int32)
        bufs = [DevBuf(cell_planes), DevBuf(n_polys), DevBuf(tasks0)]
        try:
            frx.corridor_slots_to_tasks_device(n_paths, cap_polys, cap_planes, bufs[0].p, bufs[1].p, bufs[2].p)
            tasks = bufs[2].get(tasks0)
        finally:
            for d in bufs:
                d.close()
        assert (tasks[-PAD:] == ISENT).all()
        want = slots_to_tasks_ref(n_paths, cap_polys, cap_planes, cell_planes, n_polys)
        assert np.array_equal(tasks[:-PAD].reshape(n_paths, per, 4), want), n_polys.tolist()[:4]
