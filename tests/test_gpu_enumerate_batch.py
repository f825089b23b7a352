"""frx_enumerate_vertices_batch on the device (k_enumerate, frx_enumerate_kernel.hpp) against the host's frx_enumerate_vertices on the states of
tests/enumerate_states.py: vertices, counts and statuses with == (bit for bit), the verdicts and refusals each between two healthy neighbours, the capacity
edge, the equality of the two forms, of runs and of batches, the one-node capture, the chain corridors -> tasks -> vertices on the device, and the optimiser fed
with the result.  Where the host refuses a polytope (unbounded, flat) it gives the count alone; the vertices are then held to the numpy restatement
(tests/enumerate_reference.py), which test_enumerate_states_cpu.py ties to the host on every state it accepts.

The kernel's window is 256 ranks, so the window edges are ranks 255 / 256 / 257 as the states place them; inside a window each of its four waves stages its
feasible triples in an area of its own, so ranks 63 / 64 / 65 (the edge between the first two areas) are run as well."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import corridor_states as cs  # noqa: E402
import enumerate_reference as er  # noqa: E402
import enumerate_states as es  # noqa: E402
from test_enumerate_states_cpu import corridor_polytopes  # noqa: E402
from test_gpu_trajectory_sample import DevBuf, hip  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL, ISENT, PAD = -7.0, -77, 256


def pack(polys):
    """record arrays [K][6] -> (tasks [n][4] of cells, one record array)"""
    tasks = []; at = 0
    for rec in polys:
        tasks.append([at, len(rec), 0, 0]); at += len(rec)
    return np.array(tasks, np.int32).reshape(-1, 4), np.concatenate([np.asarray(r, dtype=np.float64).reshape(-1, 6) for r in polys])


def device_enum(frx, tasks, rec, cap_v=64, launch=None, stream=0):
    """the slotted outputs of the device form (v_slot [n][cap_v][3], nv [n], status [n]); every buffer pre-filled with a sentinel and PAD entries longer than it
    has to be, the pads and everything behind a task's vertices checked to be untouched"""
    tasks = np.ascontiguousarray(tasks, dtype=np.int32).reshape(-1, 4); n = len(tasks)
    slot = np.full(n * cap_v * 3 + PAD, SENTINEL); nv = np.full(n + PAD, ISENT, np.int32); st = np.full(n + PAD, ISENT, np.int32)
    bufs = [DevBuf(tasks.reshape(-1)), DevBuf(np.ascontiguousarray(rec, dtype=np.float64).reshape(-1)), DevBuf(slot), DevBuf(nv), DevBuf(st)]
    try:
        def call():
            frx.enumerate_vertices_batch_device(n, bufs[0].p, bufs[1].p, cap_v, bufs[2].p, bufs[3].p, bufs[4].p, stream)
        (launch or (lambda f: f()))(call)
        slot_o, nv_o, st_o = bufs[2].get(slot), bufs[3].get(nv), bufs[4].get(st)
        assert (slot_o[-PAD:] == SENTINEL).all() and (nv_o[-PAD:] == ISENT).all() and (st_o[-PAD:] == ISENT).all()
        slot_o = slot_o[:-PAD].reshape(n, cap_v, 3); nv_o = nv_o[:n]; st_o = st_o[:n]
        assert ((nv_o >= 0) & (nv_o <= cap_v)).all() and ((st_o >= 0) & (st_o <= 6)).all()
        for t in range(n):
            assert (slot_o[t, nv_o[t]:] == SENTINEL).all(), t
            if st_o[t] >= frx.HV_PLANES:
                assert nv_o[t] == 0
        return slot_o, nv_o, st_o
    finally:
        for d in bufs:
            d.close()


_host = {}


def host_rows(frx, rec):
    """(nv, vertices [nv][3], status) as the device must give them: the host's count and verdict, the host's vertices where it hands them out; computed once"""
    key = np.ascontiguousarray(rec).tobytes()
    if key not in _host:
        nv, verts, verdict = er.host_enum(frx, rec)
        if verts is None:
            e = er.enumerate_ref(rec)
            assert len(e["vertices"]) == nv and e["verdict"] == verdict
            verts = e["vertices"]
        _host[key] = (nv, verts, verdict)
    return _host[key]


def assert_parity(frx, polys, cap_v=64, statuses=None):
    tasks, rec = pack(polys)
    slot, nv, st = device_enum(frx, tasks, rec, cap_v)
    for t, p in enumerate(polys):
        hn, hv, hs = host_rows(frx, p)
        assert nv[t] == hn and st[t] == hs, (t, nv[t], hn, st[t], hs)
        assert np.array_equal(slot[t, :hn], hv), (t, np.argwhere(slot[t, :hn] != hv)[:4].tolist())
    if statuses is not None:
        assert st.tolist() == statuses
    return slot, nv, st


def test_small_polytopes(frx):
    polys = [es.tetrahedron(), es.cube(), es.pyramid(8), es.pyramid(40)]
    slot, nv, st = assert_parity(frx, polys, statuses=[0, 0, 0, 0])
    assert nv.tolist() == [4, 8, 9, 41]
    e = er.enumerate_ref(es.pyramid(40))                                     # the apex: 9 880 triples of one key, the survivor is the first one's own bits
    keys = [tuple(k) for k in e["keys"]]
    apex = max(set(keys), key=keys.count)
    assert np.array_equal(slot[3, sorted(set(keys)).index(apex)], e["points"][keys.index(apex)])


def test_sphere_polytopes(frx):
    _, nv, _ = assert_parity(frx, [es.sphere(13, es.SEED_13), es.sphere(62, es.SEED_62)], cap_v=96, statuses=[0, 0])
    assert nv.tolist() == [22, 82]


def test_corridor_cells_and_overlaps(frx, sc):
    polys = corridor_polytopes(frx, sc)
    assert len(polys) >= 40 and max(len(p) for p in polys) <= 62
    assert_parity(frx, polys, statuses=[0] * len(polys))


def test_window_edges(frx):
    states = es.window_states(er.enumerate_ref)
    slot, nv, st = assert_parity(frx, [rec for _, rec, _, _ in states], statuses=[0] * len(states))
    for t, (name, rec, r, key) in enumerate(states):                          # and the vertex of the named rank is there
        keys = np.rint(slot[t, :nv[t]] / 1e-7).astype(np.int64)
        assert key in set(map(tuple, keys)), name


def test_verdicts_and_refusals_stand_between_healthy_neighbours(frx):
    left, right = es.sphere(13, es.SEED_13), es.cube()
    base, _, _ = device_enum(frx, *pack([left, right]))
    nan_rec = es.cube().copy(); nan_rec[3, 4] = np.nan
    inf_rec = es.cube().copy(); inf_rec[5, 0] = np.inf
    many = es.sphere(257, 3)
    cases = [("unbounded", es.open_cube(), frx.HV_UNBOUNDED), ("flat", es.two_cubes(), frx.HV_FLAT), ("K3", es.tetrahedron()[:3], frx.HV_PLANES),
             ("K257", many, frx.HV_PLANES), ("nan", nan_rec, frx.HV_NONFINITE), ("inf", inf_rec, frx.HV_NONFINITE), ("skipped", es.cube(), frx.HV_SKIPPED)]
    for name, mid, want in cases:
        tasks, rec = pack([left, mid, right])
        if name == "skipped":
            tasks[1, 1] = 0
        slot, nv, st = device_enum(frx, tasks, rec)
        assert st.tolist() == [0, want, 0], name
        assert np.array_equal(slot[0], base[0]) and np.array_equal(slot[2], base[1]) and nv[0] == 22 and nv[2] == 8, name
        if want in (frx.HV_UNBOUNDED, frx.HV_FLAT):                         # the host's count and verdict; the vertices as the host computes them
            hn, hv, hs = host_rows(frx, mid)
            assert hs == want and nv[1] == hn == 4 and np.array_equal(slot[1, :4], hv), name


def test_capacity(frx):
    big, left, right = es.sphere(62, es.SEED_62), es.cube(), es.tetrahedron()
    tasks, rec = pack([left, big, right])
    slot81, nv81, st81 = device_enum(frx, tasks, rec, cap_v=81)
    slot82, nv82, st82 = device_enum(frx, tasks, rec, cap_v=82)
    assert st81.tolist() == [0, frx.HV_VERTICES, 0] and nv81.tolist() == [8, 0, 4]
    assert st82.tolist() == [0, 0, 0] and nv82.tolist() == [8, 82, 4]
    assert np.array_equal(slot82[1], host_rows(frx, big)[1])
    for t in (0, 2):
        assert np.array_equal(slot81[t, :nv81[t]], slot82[t, :nv82[t]])
    # cap_vert too small on the blocking form: FRX_ERR_CAPACITY, *n_vert the need, the statuses valid
    coarse_n = np.array([2], np.int32); h_off = np.array([0, 6, 10], np.int32); h_rec = np.concatenate([left, right]).reshape(-1)
    status = np.full(3, ISENT, np.int32); v_off = np.zeros(4, np.int32); need = C.c_int(); v_rec = np.full(3 * 8, SENTINEL)
    rc = frx.lib().frx_enumerate_vertices_batch(0, 1, coarse_n.ctypes.data, h_off.ctypes.data, h_rec.ctypes.data, 16, status.ctypes.data, v_off.ctypes.data, 8,
                                                C.byref(need), v_rec.ctypes.data)
    nvs = [host_rows(frx, p)[0] for p in (left, np.concatenate([left, right]), right)]
    assert rc == -5 and need.value == sum(nvs) > 8 and status.tolist() == [0, 0, 0] and (v_rec == SENTINEL).all()


def blocking_polys(coarse_n, h_off, h_rec):
    """the polytopes of the blocking form in task order"""
    rec = np.asarray(h_rec).reshape(-1, 6); out = []; m = 0
    for n in coarse_n:
        for i in range(n):
            out.append(rec[h_off[m + i]:h_off[m + i + 1]])
            if i + 1 < n:
                out.append(rec[h_off[m + i]:h_off[m + i + 2]])
        m += n
    return out


def test_forms_runs_and_batches_give_identical_bits(frx, sc):
    w = cs.world(frx, sc)
    cells = [[np.ascontiguousarray(H.T) for H in w["ref"][i]] for i in (1, 0)]                # a one-cell corridor and a long one
    coarse_n = np.array([len(c) for c in cells], np.int32)
    flat = [rec for c in cells for rec in c]
    h_off = np.zeros(len(flat) + 1, np.int32); h_off[1:] = np.cumsum([len(r) for r in flat]); h_rec = np.concatenate(flat)
    v_off, v_rec, status = frx.enumerate_vertices_batch(coarse_n, h_off, h_rec)
    polys = blocking_polys(coarse_n, h_off, h_rec)
    assert len(status) == len(polys) == 2 * coarse_n.sum() - 2 and status.tolist() == [0] * len(polys)
    slot, nv, st = device_enum(frx, *pack(polys))
    assert np.array_equal(st, status) and np.array_equal(np.concatenate([[0], np.cumsum(nv)]), v_off)
    assert np.array_equal(np.concatenate([slot[t, :nv[t]].reshape(-1) for t in range(len(polys))]), v_rec)       # blocking form == compacted device form
    again = frx.enumerate_vertices_batch(coarse_n, h_off, h_rec)
    assert all(np.array_equal(x, y) for x, y in zip(again, (v_off, v_rec, status)))
    slot2, nv2, st2 = device_enum(frx, *pack(polys))
    assert np.array_equal(slot2, slot) and np.array_equal(nv2, nv) and np.array_equal(st2, st)
    # a task alone == the same task anywhere in a shuffled batch
    order = np.random.default_rng(4).permutation(len(polys))
    slot3, nv3, st3 = device_enum(frx, *pack([polys[i] for i in order]))
    for pos, i in enumerate(order):
        assert nv3[pos] == nv[i] and np.array_equal(slot3[pos], slot[i])
    alone, nva, _ = device_enum(frx, *pack([polys[5]]))
    assert nva[0] == nv[5] and np.array_equal(alone[0], slot[5])


def test_device_form_is_one_graph_node(frx):
    """no copy, no synchronisation, no allocation: the call is captured as a single kernel node and the replayed graph writes the same bits"""
    tasks, rec = pack([es.cube(), es.sphere(13, es.SEED_13), es.pyramid(8)])
    want = device_enum(frx, tasks, rec)
    H = hip()
    st = C.c_void_p(); graph = C.c_void_p(); exe = C.c_void_p(); n = C.c_size_t()
    assert H.hipStreamCreate(C.byref(st)) == 0

    def captured(call):
        assert H.hipStreamBeginCapture(st, 0) == 0                          # hipStreamCaptureModeGlobal
        call()
        assert H.hipStreamEndCapture(st, C.byref(graph)) == 0
        assert H.hipGraphGetNodes(graph, None, C.byref(n)) == 0 and n.value == 1
        assert H.hipGraphInstantiate(C.byref(exe), graph, None, None, 0) == 0
        assert H.hipGraphLaunch(exe, st) == 0 and H.hipStreamSynchronize(st) == 0
    try:
        got = device_enum(frx, tasks, rec, launch=captured, stream=st.value)
        assert all(np.array_equal(x, y) for x, y in zip(got, want))
    finally:
        if exe.value:
            H.hipGraphExecDestroy(exe)
        if graph.value:
            H.hipGraphDestroy(graph)
        H.hipStreamDestroy(st)


def test_the_chain_on_the_device(frx, sc):
    """corridors -> tasks -> vertices without the host: the corridor generator's slots, the task kernel, the enumeration; judged on the device-made records"""
    w = cs.world(frx, sc)
    paths = [w["paths"][i] for i in (0, 1, 3)]; cloud, vm = w["cloud"], w["vm"]
    cap_polys, cap_planes, cap_v, B = 64, 96, 64, 3
    per = 2 * cap_polys - 1
    off = np.zeros(B + 1, np.int32); off[1:] = np.cumsum([len(p) for p in paths])
    hslot0 = np.full(B * cap_polys * cap_planes * 6, SENTINEL); cp0 = np.full(B * cap_polys, ISENT, np.int32); np0 = np.full(B, ISENT, np.int32)
    tasks0 = np.full(B * per * 4 + PAD, ISENT, np.int32)
    slot0 = np.full(B * per * cap_v * 3 + PAD, SENTINEL); nv0 = np.full(B * per + PAD, ISENT, np.int32); st0 = np.full(B * per + PAD, ISENT, np.int32)
    bufs = [DevBuf(off), DevBuf(np.concatenate(paths).reshape(-1)), DevBuf(np.ascontiguousarray(cloud).reshape(-1)), DevBuf(vm.cells), DevBuf(hslot0), DevBuf(cp0),
            DevBuf(np0), DevBuf(np0), DevBuf(tasks0), DevBuf(slot0), DevBuf(nv0), DevBuf(st0)]
    ms = frx.VoxelMapStruct((C.c_double * 3)(*vm.origin), (C.c_int * 3)(*[int(d) for d in vm.dim]), vm.res, bufs[3].p)
    try:                                                                    # three launches on the null stream, nothing in between
        frx.corridor_generate_batch_device(B, bufs[0].p, bufs[1].p, len(cloud), bufs[2].p, cs.BBOX, cs.MAP_HEIGHT, cs.MAX_SEG, ms, cap_polys, cap_planes, bufs[4].p,
                                           bufs[5].p, bufs[6].p, bufs[7].p)
        frx.corridor_slots_to_tasks_device(B, cap_polys, cap_planes, bufs[5].p, bufs[6].p, bufs[8].p)
        frx.enumerate_vertices_batch_device(B * per, bufs[8].p, bufs[4].p, cap_v, bufs[9].p, bufs[10].p, bufs[11].p)
        hslot, cp, npol, cst = bufs[4].get(hslot0), bufs[5].get(cp0), bufs[6].get(np0), bufs[7].get(np0)
        tasks, slot, nv, st = bufs[8].get(tasks0), bufs[9].get(slot0), bufs[10].get(nv0), bufs[11].get(st0)
    finally:
        for d in bufs:
            d.close()
    hslot = hslot.reshape(B, cap_polys, cap_planes, 6); cp = cp.reshape(B, cap_polys)
    assert cst.tolist() == [0, 0, 0] and npol[1] == 1 and 4 <= npol.max() <= cap_polys
    assert (tasks[-PAD:] == ISENT).all() and (slot[-PAD:] == SENTINEL).all() and (nv[-PAD:] == ISENT).all() and (st[-PAD:] == ISENT).all()
    tasks = tasks[:-PAD].reshape(B, per, 4); slot = slot[:-PAD].reshape(B, per, cap_v, 3); nv = nv[:-PAD].reshape(B, per); st = st[:-PAD].reshape(B, per)
    for b in range(B):
        n = int(npol[b])
        for q in range(per):
            c = q // 2
            if q >= 2 * n - 1:
                assert tasks[b, q].tolist() == [0, 0, 0, 0] and st[b, q] == frx.HV_SKIPPED and nv[b, q] == 0 and (slot[b, q] == SENTINEL).all()
                continue
            rec = hslot[b, c, :cp[b, c]]                                     # a cell's records are its own, an overlap's the two cells' concatenated
            want = [(b * cap_polys + c) * cap_planes, cp[b, c], 0, 0]
            if q % 2:
                rec = np.concatenate([rec, hslot[b, c + 1, :cp[b, c + 1]]])
                want[2:] = [(b * cap_polys + c + 1) * cap_planes, cp[b, c + 1]]
            assert tasks[b, q].tolist() == want
            hn, hv, hs = host_rows(frx, rec)
            assert st[b, q] == hs == 0 and nv[b, q] == hn and np.array_equal(slot[b, q, :hn], hv), (b, q)
            assert (slot[b, q, hn:] == SENTINEL).all()


def test_vertices_feed_the_optimiser(frx, sc):
    cands = sc.make_batch(1, 4, 16, 4)
    coarse_n, ini, fin, h_off, h_rec, _, _ = frx.pack_batch(cands)
    v_off, v_rec, status = frx.enumerate_vertices_batch(coarse_n, h_off, h_rec)
    assert status.tolist() == [0] * len(status) and len(v_off) == 2 * coarse_n.sum() - len(cands) + 1
    mine = frx.Problem(cands, sc.ZHANGJIAJIE, packed=(coarse_n, ini, fin, h_off, h_rec, v_off, v_rec), qd_intervals=8)
    host = frx.Problem(cands, sc.ZHANGJIAJIE, enumerate_v=True, packed=(coarse_n, ini, fin, h_off, h_rec, None, None), qd_intervals=8)
    try:
        x0, x1 = mine.initial_guess(), host.initial_guess()
        assert np.array_equal(x0, x1)
        (f0, g0), (f1, g1) = mine.objective(x0), host.objective(x1)
        assert np.array_equal(f0, f1) and np.array_equal(g0, g1)
    finally:
        mine.close(); host.close()
