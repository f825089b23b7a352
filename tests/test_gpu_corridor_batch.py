"""frx_corridor_generate_batch on the device (k_corridor_chain, frx_chain_kernel.hpp) against the host chain frx_corridor_generate path by path on the decision-safe
scenes of tests/corridor_states.py: same number of cells, same plane count per cell, canonically sorted planes within 1e-9 (what test_next_rows.py holds k_dilate
to against the host form); sight-line verdicts, independence of the batch, run-to-run identity and the equality of the two forms with ==."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import corridor_states as cs  # noqa: E402
from test_gpu_trajectory_sample import DevBuf, hip  # noqa: E402
from test_next_rows import _canon  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = 1e-9
SENTINEL, ISENT, PAD = -7.0, -77, 256


def assert_same_corridor(got, want, who=""):
    assert len(got) == len(want), (who, len(got), len(want))
    for c, (H, Hw) in enumerate(zip(got, want)):
        assert H.shape == Hw.shape, (who, c, H.shape, Hw.shape)
        assert np.array_equal(H[:, -2:], Hw[:, -2:])                        # ceiling, then floor, last
        assert np.abs(_canon(H[:, :-2]) - _canon(Hw[:, :-2])).max() < TOL, (who, c)


@pytest.fixture(scope="module")
def w(frx, sc):
    return cs.world(frx, sc)


@pytest.mark.parametrize("ids", [[0], [1, 4], list(range(9))], ids=["one", "two", "nine"])
@pytest.mark.parametrize("with_map", [True, False], ids=["map", "free"])
def test_batch_matches_the_host_chain(frx, ob, w, ids, with_map):
    paths = [w["paths"][i] for i in ids]
    got, st = frx.corridor_generate_batch(paths, w["cloud"], cs.BBOX, cs.MAP_HEIGHT, cs.MAX_SEG, blocked=w["vm"] if with_map else None)
    assert st.tolist() == [0] * len(ids)
    for i, g in zip(ids, got):
        assert_same_corridor(g, (w["ref"] if with_map else w["ref_free"])[i], f"path {i}")
    if ob.ref_decomp() is not None:                                         # the reference's own decomp_util under the restated loop
        blocked = (lambda a, b: w["vm"].is_blocked(a, b)) if with_map else None
        for i, g in list(zip(ids, got))[:2]:
            assert_same_corridor(g, ob.corridor_oracle(w["paths"][i], w["cloud"], cs.BBOX, cs.MAP_HEIGHT, cs.MAX_SEG, blocked=blocked), f"path {i} (reference)")


@pytest.mark.parametrize("seed,gates,n_obs", [(11, 1, 400), (12, 2, 1200)])
def test_small_scenes(frx, sc, seed, gates, n_obs):
    path, cloud, vm = cs.small_scene(frx, sc, seed, gates, n_obs)
    (got,), st = frx.corridor_generate_batch([path], cloud, cs.BBOX, cs.MAP_HEIGHT, cs.MAX_SEG, blocked=vm)
    assert st.tolist() == [0]
    assert_same_corridor(got, frx.corridor_generate(path, cloud, cs.BBOX, cs.MAP_HEIGHT, cs.MAX_SEG, blocked=vm))


def test_sight_lines_equal_the_host_verdicts(frx):
    vm = cs.sight_map(frx)
    for name, (a, b) in cs.sight_pairs(vm).items():
        want = np.array([vm.is_blocked(p, q) for p, q in zip(a, b)])
        got = vm.is_blocked_device(a, b)
        assert np.array_equal(got, want), (name, np.argwhere(got != want)[:5].ravel())


def device_form(frx, paths, cloud, vm, cap_polys=64, cap_planes=96, bbox=cs.BBOX, max_seg=cs.MAX_SEG, launch=None, stream=0):
    """the slotted outputs of the device form, every buffer pre-filled with a sentinel and PAD entries longer than it has to be"""
    B = len(paths)
    off = np.zeros(B + 1, np.int32); off[1:] = np.cumsum([len(p) for p in paths])
    slot = np.full(B * cap_polys * cap_planes * 6 + PAD, SENTINEL); cp = np.full(B * cap_polys + PAD, ISENT, np.int32)
    npol = np.full(B + PAD, ISENT, np.int32); st = np.full(B + PAD, ISENT, np.int32)
    bufs = [DevBuf(off), DevBuf(np.concatenate(paths).reshape(-1)), DevBuf(np.ascontiguousarray(cloud).reshape(-1)), DevBuf(slot), DevBuf(cp), DevBuf(npol), DevBuf(st)]
    ms = None
    if vm is not None:
        bufs.append(DevBuf(vm.cells))
        ms = frx.VoxelMapStruct((C.c_double * 3)(*vm.origin), (C.c_int * 3)(*[int(d) for d in vm.dim]), vm.res, bufs[-1].p)
    try:
        def call():
            frx.corridor_generate_batch_device(B, bufs[0].p, bufs[1].p, len(cloud), bufs[2].p, bbox, cs.MAP_HEIGHT, max_seg, ms, cap_polys, cap_planes,
                                               bufs[3].p, bufs[4].p, bufs[5].p, bufs[6].p, stream)
        (launch or (lambda f: f()))(call)
        slot_o, cp_o, np_o, st_o = bufs[3].get(slot), bufs[4].get(cp), bufs[5].get(npol), bufs[6].get(st)
        assert (slot_o[-PAD:] == SENTINEL).all() and (cp_o[-PAD:] == ISENT).all() and (np_o[-PAD:] == ISENT).all() and (st_o[-PAD:] == ISENT).all()
        slot_o = slot_o[:-PAD].reshape(B, cap_polys, cap_planes, 6); cp_o = cp_o[:-PAD].reshape(B, cap_polys)
        for b in range(B):                                                  # and nothing behind a path's cells or a cell's records
            assert (cp_o[b, np_o[b]:] == ISENT).all() and (slot_o[b, np_o[b]:] == SENTINEL).all()
            for c in range(np_o[b]):
                assert (slot_o[b, c, cp_o[b, c]:] == SENTINEL).all()
        return slot_o, cp_o, np_o[:B], st_o[:B]
    finally:
        for d in bufs:
            d.close()


def compact(slot, cp, npol):
    """what the blocking form does with the slots: (h_off, h_rec)"""
    h_off = [0]; rec = []
    for b in range(len(npol)):
        for c in range(npol[b]):
            rec.append(slot[b, c, :cp[b, c]].reshape(-1)); h_off.append(h_off[-1] + int(cp[b, c]))
    return np.array(h_off, np.int32), np.concatenate(rec)


def test_forms_runs_and_batches_give_identical_bits(frx, w):
    paths, cloud, vm = w["paths"], w["cloud"], w["vm"]
    n9, off9, rec9, st9 = frx.corridor_generate_batch(paths, cloud, cs.BBOX, cs.MAP_HEIGHT, cs.MAX_SEG, blocked=vm, raw=True)
    slot, cp, npol, st = device_form(frx, paths, cloud, vm)
    assert np.array_equal(npol, n9) and np.array_equal(st, st9) and st.tolist() == [0] * 9
    h_off, h_rec = compact(slot, cp, npol)
    assert np.array_equal(h_off, off9) and np.array_equal(h_rec, rec9)      # blocking form == compacted device form, bit for bit
    again = frx.corridor_generate_batch(paths, cloud, cs.BBOX, cs.MAP_HEIGHT, cs.MAX_SEG, blocked=vm, raw=True)
    assert all(np.array_equal(x, y) for x, y in zip(again, (n9, off9, rec9, st9)))
    n1, off1, rec1, st1 = frx.corridor_generate_batch(paths[:1], cloud, cs.BBOX, cs.MAP_HEIGHT, cs.MAX_SEG, blocked=vm, raw=True)
    assert n1[0] == n9[0] and np.array_equal(off1, off9[:n1[0] + 1]) and np.array_equal(rec1, rec9[:6 * off9[n1[0]]])      # path 0 alone == path 0 among nine
    # any order of the batch: a path's rows do not depend on where it stands
    order = [8, 0, 4, 1, 7, 2, 6, 3, 5]
    got, _ = frx.corridor_generate_batch([paths[i] for i in order], cloud, cs.BBOX, cs.MAP_HEIGHT, cs.MAX_SEG, blocked=vm)
    ref = frx.unpack_corridors(n9, off9, rec9)
    for i, g in zip(order, got):
        assert len(g) == len(ref[i]) and all(np.array_equal(x, y) for x, y in zip(g, ref[i]))


def test_device_form_is_one_graph_node(frx, w):
    """no copy, no synchronisation, no allocation: the call is captured as a single kernel node and the replayed graph writes the same slots"""
    paths, cloud, vm = w["paths"][:3], w["cloud"], w["vm"]
    want = device_form(frx, paths, cloud, vm)                                # (also the first launch of the process's kernel, outside a capture)
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
        got = device_form(frx, paths, cloud, vm, launch=captured, stream=st.value)
        assert all(np.array_equal(x, y) for x, y in zip(got, want))
    finally:
        if exe.value:
            H.hipGraphExecDestroy(exe)
        if graph.value:
            H.hipGraphDestroy(graph)
        H.hipStreamDestroy(st)


def test_each_overflow_leaves_the_neighbours_alone(frx, sc, w):
    paths, vm = w["paths"], w["vm"]
    two, fogged, scene = paths[1], paths[4], paths[3]
    # 1: more than 4096 cloud points in one cell's local box
    lone, cloud5k = cs.clump_world(frx, sc)
    trio = [paths[0], lone, paths[2]]
    got, st = frx.corridor_generate_batch(trio, cloud5k, cs.BBOX, cs.MAP_HEIGHT, cs.MAX_SEG, blocked=vm)
    assert st.tolist() == [0, frx.CHAIN_BOX_POINTS, 0] and got[1] == []
    alone, st2 = frx.corridor_generate_batch([paths[0], paths[2]], cloud5k, cs.BBOX, cs.MAP_HEIGHT, cs.MAX_SEG, blocked=vm)
    assert st2.tolist() == [0, 0]
    for g, a in zip((got[0], got[2]), alone):
        assert len(g) == len(a) and all(np.array_equal(x, y) for x, y in zip(g, a))
    assert_same_corridor(got[0], w["ref"][0]); assert_same_corridor(got[2], w["ref"][2])       # the clump is outside their boxes: the world's corridors
    # 2: cap_planes too small for a cell among obstacles, enough for the cells in free space (local box, floor, ceiling = 8)
    assert max(H.shape[1] for H in w["ref"][3]) > 8
    got, st = frx.corridor_generate_batch([two, scene, fogged], w["cloud"], cs.BBOX, cs.MAP_HEIGHT, cs.MAX_SEG, blocked=vm, cap_planes=8)
    assert st.tolist() == [0, frx.CHAIN_PLANES, 0] and got[1] == []
    wide, _ = frx.corridor_generate_batch([two, fogged], w["cloud"], cs.BBOX, cs.MAP_HEIGHT, cs.MAX_SEG, blocked=vm, cap_planes=96)
    for g, a in zip((got[0], got[2]), wide):
        assert len(g) == len(a) >= 1 and all(np.array_equal(x, y) for x, y in zip(g, a))
    # 3: cap_polys = 1
    short = np.array([[25.0, 40.0, 1.0], [25.0, 42.5, 1.2], [25.0, 43.0, 1.4]])
    got, st = frx.corridor_generate_batch([two, scene, short], w["cloud"], cs.BBOX, cs.MAP_HEIGHT, cs.MAX_SEG, blocked=vm, cap_polys=1)
    assert st.tolist() == [0, frx.CHAIN_POLYS, 0] and got[1] == [] and len(got[0]) == len(got[2]) == 1
    roomy, _ = frx.corridor_generate_batch([two, short], w["cloud"], cs.BBOX, cs.MAP_HEIGHT, cs.MAX_SEG, blocked=vm)
    for g, a in zip((got[0], got[2]), roomy):
        assert len(g) == len(a) == 1 and np.array_equal(g[0], a[0])
    # and cap_rec: too small reports the need and FRX_ERR_CAPACITY, n_polys and status still valid
    n_polys = np.zeros(1, np.int32); status = np.zeros(1, np.int32); h_off = np.zeros(65, np.int32); h_rec = np.zeros(6 * 4); need = C.c_int()
    off = np.array([0, len(scene)], np.int32); flat = np.ascontiguousarray(scene.reshape(-1)); cl = np.ascontiguousarray(w["cloud"].reshape(-1))
    rc = frx.lib().frx_corridor_generate_batch(0, 1, off.ctypes.data, flat.ctypes.data, len(w["cloud"]), cl.ctypes.data, cs.BBOX.ctypes.data, cs.MAP_HEIGHT, cs.MAX_SEG,
                                               C.addressof(vm._s), 64, 96, n_polys.ctypes.data, status.ctypes.data, 4, C.byref(need), h_off.ctypes.data, h_rec.ctypes.data)
    assert rc == -5 and need.value == sum(H.shape[1] for H in w["ref"][3]) and n_polys[0] == len(w["ref"][3]) and status[0] == 0


@pytest.mark.parametrize("case", range(6))
def test_window_edges(frx, case):
    """the first stop (cases 0-2) or the exit index (3-5) on lane 255 of a window of 256 path points, lane 0 and lane 1 of the next"""
    path, cloud = cs.dense_scene(frx)
    ms, bx = cs.EDGE_CASES[case]
    bbox = np.array([bx, 4.0, 2.5])
    (got,), st = frx.corridor_generate_batch([path], cloud, bbox, cs.MAP_HEIGHT, ms)
    assert st.tolist() == [0]
    assert_same_corridor(got, frx.corridor_generate(path, cloud, bbox, cs.MAP_HEIGHT, max_seg=ms))


def test_corridors_feed_the_optimiser(frx, sc, w):
    ids = [0, 2, 3]
    paths = [w["paths"][i] for i in ids]
    n_polys, h_off, h_rec, st = frx.corridor_generate_batch(paths, w["cloud"], cs.BBOX, cs.MAP_HEIGHT, cs.MAX_SEG, blocked=w["vm"], raw=True)
    assert st.tolist() == [0, 0, 0] and n_polys.min() >= 4
    zero = np.zeros(6)
    ini = np.concatenate([np.concatenate([p[0], zero]) for p in paths]); fin = np.concatenate([np.concatenate([p[-1], zero]) for p in paths])
    prob = frx.Problem([None] * len(paths), sc.ZHANGJIAJIE, enumerate_v=True, packed=(n_polys, ini, fin, h_off, h_rec, None, None), qd_intervals=8)
    try:
        res = prob.optimize(1e-4, max_iterations=15)
        assert np.all(np.isfinite(res["C"])) and np.all(np.isfinite(res["T"])) and np.all(np.isfinite(res["objective"])) and np.all(res["T"] > 0)
    finally:
        prob.close()
