"""The canonical level search of the route batch on the host (frx_grid_search_levels, frx_route_plan_levels_batch; csrc/frx_route_host.hpp)
against its definition: the properties of a shortest face-neighbour path, the integer cost of the reference's own search (frx_grid_search, eps = 1), and a numpy
restatement cell for cell (tests/route_reference.py); the batch against the restatement's spliced routes bit for bit; the exact capacities; and the argument
rules, all without a device."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import route_reference as rr  # noqa: E402

DIM = (24, 40, 6)
RES = 0.1
ORIGIN = (-1.2, -2.0, 0.0)


def free_cell(rng, cells, dim):
    return rr.free_cell(rng, cells, dim)


def check_path(frx, cells, dim, s, g):
    path, levels, mx = frx.grid_search_levels(cells, dim, s, g)
    st, want, wl, wm = rr.level_search(cells, dim, s, g)
    assert st == rr.OK and levels == wl and mx == wm
    assert len(path) == levels + 1 and list(path[0]) == list(s) and list(path[-1]) == list(g)
    assert (np.abs(np.diff(path, axis=0)).sum(axis=1) == 1).all()                                   # face neighbours
    assert (path >= 0).all() and (path < np.array(dim)).all()
    assert (cells[path[:, 0] + dim[0] * path[:, 1] + dim[0] * dim[1] * path[:, 2]] <= 0).all()       # through traversable cells
    assert [tuple(p) for p in path] == want                                                          # the restatement, cell for cell
    ref, _, cost = frx.grid_search((cells > 0).astype(np.int8), dim, s, g, eps=1.0, use_jps=False)
    assert len(ref) == levels + 1 and cost == float(levels) and int(cost) == levels                  # the reference's length, as an integer
    return levels, mx


def test_random_pairs_are_shortest_paths_and_equal_the_restatement(frx):
    rng = np.random.default_rng(11)
    seen_levels, seen_cells, n = 0, 0, 0
    for k in range(6):
        cells = rr.box_map(rng, DIM, 0.03 + 0.004 * k)
        for _ in range(40):
            s, g = free_cell(rng, cells, DIM), free_cell(rng, cells, DIM)
            if rr.level_search(cells, DIM, s, g)[0] != rr.OK:
                continue                                                                            # walled in by boxes: the edge cases cover it
            levels, mx = check_path(frx, cells, DIM, s, g)
            seen_levels = max(seen_levels, levels); seen_cells = max(seen_cells, mx); n += 1
    assert n >= 200 and seen_levels >= 30 and seen_cells >= 100


def test_edge_cases_of_the_search(frx):
    dim = (7, 9, 3)                                                                                 # dim[0] not divisible by 4
    cells = np.zeros(dim[::-1], np.int8)
    cells[:, 4, :] = 100                                                                            # a sealed wall across y = 4
    flat = cells.reshape(-1)
    path, levels, mx = frx.grid_search_levels(flat, dim, [1, 1, 1], [5, 7, 1])
    assert len(path) == 0 and levels == -1 and mx == rr.level_search(flat, dim, [1, 1, 1], [5, 7, 1])[3]
    assert rr.level_search(flat, dim, [1, 1, 1], [5, 7, 1])[0] == rr.NO_PATH
    cells[1, 4, 3] = -1                                                                             # an unknown cell is the only way through
    check_path(frx, flat, dim, [1, 1, 1], [5, 7, 1])
    path, _, _ = frx.grid_search_levels(flat, dim, [1, 1, 1], [5, 7, 1])
    assert [3, 4, 1] in path.tolist()
    path, levels, mx = frx.grid_search_levels(flat, dim, [2, 2, 2], [2, 2, 2])                      # start = goal: one cell
    assert path.tolist() == [[2, 2, 2]] and levels == 0 and mx == 1
    for s, g in (([3, 4, 0], [1, 1, 1]), ([1, 1, 1], [3, 4, 0])):                                   # an occupied end
        path, levels, _ = frx.grid_search_levels(flat, dim, s, g)
        assert len(path) == 0 and levels == -1
    check_path(frx, flat, dim, [6, 0, 0], [0, 3, 2])
    check_path(frx, flat, dim, [0, 8, 2], [6, 5, 0])


@pytest.fixture(scope="module")
def batch():
    """One map; routes with 0 and 3 gates, one with a gate inside a box, one that starts and one that ends in an unknown cell, one that ends in a walled-in
    cell; and the restatement's answer: computed once, shared, left unchanged."""
    cells, routes = rr.mixed_batch(DIM, ORIGIN, RES)
    ref = rr.route_batch(rr.Map(ORIGIN, DIM, RES, cells), routes)
    cells.setflags(write=False)
    return cells, routes, ref


def assert_same_batch(got, want, label=""):
    assert list(got["route_status"]) == list(want["route_status"]), label
    assert list(got["leg_status"]) == list(want["leg_status"]), label
    assert list(got["levels"]) == list(want["levels"]) and list(got["max_level_cells"]) == list(want["max_level_cells"]), label
    assert len(got["paths"]) == len(want["paths"])
    for r, (a, b) in enumerate(zip(got["paths"], want["paths"])):
        assert rr.same_bits(a, b), (label, r)


def test_batch_equals_the_restatement_bit_for_bit(frx, batch):
    cells, routes, ref = batch
    m = frx.VoxelMap(ORIGIN, DIM, RES, cells)
    got = m.route_batch_host(routes)
    assert list(ref["route_status"]) == rr.MIXED_ROUTE_STATUS
    assert {k: int(v) for k, v in enumerate(ref["leg_status"]) if v != 0} == rr.MIXED_LEG_FAILURES   # 2, 1 at the box; 1 and 2 at the unknown ends; -1 behind the wall
    om = rr.Map(ORIGIN, DIM, RES, cells)
    assert cells[om.index(om.float_to_int(routes[5][0]))] == -1 and cells[om.index(om.float_to_int(routes[6][-1]))] == -1   # the ends that are unknown cells
    assert (cells == -1).sum() > 40 and ref["levels"][14] == -1 and ref["max_level_cells"][14] == 1  # the walled-in goal: level 0 alone
    for r in (2, 5, 6, 7):
        assert rr.same_bits(ref["paths"][r], routes[r][[0, -1]]) and rr.same_bits(got["paths"][r], routes[r][[0, -1]])   # the placeholder
    assert_same_batch(got, ref)
    assert got["fits"] and got["need"] == ref["need"] == got["path_off"][-1]
    assert list(got["path_off"]) == [0] + list(np.cumsum([len(p) for p in ref["paths"]]))
    leg = 0
    for r, wp in enumerate(routes):                                                                 # every route alone = itself inside the batch
        one = m.route_batch_host([wp])
        n = len(wp) - 1
        assert rr.same_bits(one["paths"][0], got["paths"][r]) and list(one["leg_status"]) == list(got["leg_status"][leg:leg + n])
        assert list(one["levels"]) == list(got["levels"][leg:leg + n]) and list(one["max_level_cells"]) == list(got["max_level_cells"][leg:leg + n])
        leg += n


def test_capacities_are_exact(frx, batch):
    cells, routes, ref = batch
    m = frx.VoxelMap(ORIGIN, DIM, RES, cells)
    full = m.route_batch_host(routes)
    legs_of_1 = slice(1, 5)                                                                         # route 1: three gates, four legs
    worst = int(np.argmax(full["max_level_cells"][legs_of_1])) + 1
    cap = int(full["max_level_cells"][worst])
    assert_same_batch(m.route_batch_host(routes, cap_level=int(full["max_level_cells"].max())), ref, "cap_level = the largest level")
    got = m.route_batch_host(routes, cap_level=cap - 1)
    assert got["leg_status"][worst] == 3 and got["route_status"][1] == 1 and rr.same_bits(got["paths"][1], routes[1][[0, -1]])
    want = rr.route_batch(rr.Map(ORIGIN, DIM, RES, cells), routes, cap_level=cap - 1)
    assert_same_batch(got, want, "cap_level one short")
    deepest = int(np.argmax(full["levels"]))
    D = int(full["levels"][deepest])
    assert_same_batch(m.route_batch_host(routes, cap_raw=D + 1), ref, "cap_raw = the longest raw path")
    got = m.route_batch_host(routes, cap_raw=D)
    assert got["leg_status"][deepest] == 4 and got["levels"][deepest] == D
    assert_same_batch(got, rr.route_batch(rr.Map(ORIGIN, DIM, RES, cells), routes, cap_raw=D), "cap_raw one short")
    single = m.route_batch_host([routes[0]])
    n0 = len(single["paths"][0])
    assert_same_batch(m.route_batch_host([routes[0]], cap_pts=n0), single, "cap_pts = the leg's points")
    got = m.route_batch_host([routes[0]], cap_pts=n0 - 1)
    assert list(got["leg_status"]) == [5] and list(got["route_status"]) == [1] and rr.same_bits(got["paths"][0], routes[0][[0, -1]])
    # cap_total: the sum fits; one point short, the last whole route takes its placeholder and the routes before it stay as they were
    total = int(full["path_off"][-1])
    assert_same_batch(m.route_batch_host(routes, cap_total=total), ref, "cap_total = the sum")
    got = m.route_batch_host(routes, cap_total=total - 1)
    assert not got["fits"] and got["need"] == total
    assert list(got["route_status"]) == [0, 0, 1, 0, 2, 1, 1, 1] and rr.same_bits(got["paths"][4], routes[4][[0, -1]])
    for r in range(4):
        assert rr.same_bits(got["paths"][r], full["paths"][r])
    assert_same_batch(got, rr.route_batch(rr.Map(ORIGIN, DIM, RES, cells), routes, cap_total=total - 1), "cap_total one short")


def test_workspace_and_argument_errors_need_no_device(frx, batch):
    cells, routes, _ = batch
    n = int(np.prod(DIM))
    legs, cl, cr, cp = 7, 300, 90, 500
    up8 = lambda b: (b + 7) // 8 * 8                                                                # noqa: E731
    want = up8(up8(up8(24 * cp * legs) + 4 * legs) + 4 * (2 * cl + cr) * legs)
    want = up8(want + 4 * ((n + 3) // 4) * legs)
    assert frx.route_search_workspace(DIM, legs, cl, cr, cp) == want
    assert frx.route_search_workspace((23, 3, 1), 1, 1, 1, 1) == 24 + 8 + 16 + 4 * 18               # 69 cells: 18 label words
    for bad in ((0, 4, 4), (4, -1, 4), (1 << 16, 1 << 16, 1)):
        with pytest.raises(frx.FrxError) as e:
            frx.route_search_workspace(bad, 1, 1, 1, 1)
        assert e.value.code == -1
    for args in ((0, 1, 1, 1), (1, 0, 1, 1), (1, 1, 0, 1), (1, 1, 1, 0)):
        with pytest.raises(frx.FrxError) as e:
            frx.route_search_workspace(DIM, *args)
        assert e.value.code == -1
    L = frx.lib()
    m = frx.VoxelMap(ORIGIN, DIM, RES, cells)
    off, pts = frx.pack_routes(routes)
    R, NL = len(routes), int(off[-1]) - len(routes)
    outs = [np.zeros(R + 1, np.int32), np.zeros((4096, 3)), np.zeros(R, np.int32), np.zeros(NL, np.int32), np.zeros(NL, np.int32), np.zeros(NL, np.int32)]
    need = C.c_int()

    def call(entry, ms=m._s, n_routes=R, off_=off, pts_=pts, caps=(64, 64, 64, 4096), drop=None):
        o = [a.ctypes.data for a in outs] + [C.addressof(need)]
        if drop is not None:
            o[drop] = None
        head = (0,) if entry == "frx_route_plan_batch" else ()
        return getattr(L, entry)(*head, C.byref(ms) if ms is not None else None, n_routes, off_.ctypes.data if off_ is not None else None,
                                 pts_.ctypes.data if pts_ is not None else None, *caps, *o)

    for entry in ("frx_route_plan_levels_batch", "frx_route_plan_batch"):
        assert call(entry, ms=None) == -1 and call(entry, off_=None) == -1 and call(entry, pts_=None) == -1
        for k in range(7):
            assert call(entry, drop=k) == -1, (entry, k)
        assert call(entry, n_routes=0) == -1
        for k in range(3):
            caps = [64, 64, 64, 4096]; caps[k] = 0
            assert call(entry, caps=tuple(caps)) == -1
        assert call(entry, caps=(64, 64, 64, 2 * R - 1)) == -1 and b"cap_total" in L.frx_last_error()
        short = off.copy(); short[2] = short[1] + 1
        assert call(entry, off_=short) == -1 and b"fewer than 2" in L.frx_last_error()
        back = off.copy(); back[2] = back[1] - 1
        assert call(entry, off_=back) == -1 and b"monotone" in L.frx_last_error()
        for res, dim in ((0.0, DIM), (RES, (24, 0, 6)), (RES, (1 << 16, 1 << 16, 1))):
            bad = frx.VoxelMapStruct((C.c_double * 3)(*ORIGIN), (C.c_int * 3)(*dim), res, cells.ctypes.data)
            assert call(entry, ms=bad) == -1, (entry, res, dim)
        nocells = frx.VoxelMapStruct((C.c_double * 3)(*ORIGIN), (C.c_int * 3)(*DIM), RES, None)
        assert call(entry, ms=nocells) == -1
    # the device form: the same rules before a device is looked for (addresses are not dereferenced by a refusal)
    ms = m.device_struct(1 << 20)
    good = dict(n_routes=R, n_legs=NL, pt_off_dev=8, pts_dev=8, cap_level=64, cap_raw=64, cap_pts=64, cap_total=4096, work_dev=8, path_off_dev=8, path_dev=8,
                route_status_dev=8, leg_status_dev=8, leg_levels_dev=8, leg_max_level_dev=8)
    for key, val in [(k, 0) for k in good if k.endswith("_dev")] + [("n_routes", 0), ("cap_level", 0), ("cap_raw", 0), ("cap_pts", 0), ("cap_total", 2 * R - 1),
                                                                    ("n_legs", R - 1), ("work_dev", 12)]:
        with pytest.raises(frx.FrxError) as e:
            frx.route_plan_batch_device(ms, **{**good, key: val})
        assert e.value.code == -1, key
    with pytest.raises(frx.FrxError) as e:
        frx.route_plan_batch_device(m.device_struct(0), **good)
    assert e.value.code == -1
    if L.frx_device_count() < 1:
        assert call("frx_route_plan_batch") == -2 and b"no HIP device" in L.frx_last_error()
        with pytest.raises(frx.FrxError) as e:
            frx.route_plan_batch_device(ms, **good)
        assert e.value.code == -2
