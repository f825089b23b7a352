"""frx_route_plan_window_batch and frx_route_plan_window_batch_device against the host referee (VoxelMap.route_batch_window_host =
frx_route_plan_levels_window_batch), entry for entry: every point, offset, status, levels, max_level_cells and leg_window row.  A mixed batch at three pads;
windows at the edges of the label words; a level wider than two passes of the workgroup; windows clipped at a map corner; the certificate on its edge; every
status at its exact capacity with the neighbours untouched; a caller's stream, twice, and a captured graph replayed on a workspace nobody prepared; and the
fall-back to the whole-map form."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import route_reference as rr  # noqa: E402
from test_gpu_trajectory_sample import DevBuf, hip  # noqa: E402

pytestmark = pytest.mark.gpu

THREADS = 256                                                             # ROUTE_THREADS of csrc/frx_route_kernel.hpp
SENTINEL, ISENT, PAD = -7.0, -7, 64
RES = 0.1
KEYS = ("path_off", "route_status", "leg_status", "levels", "max_level_cells", "leg_window")
BIG = dict(cap_level=1 << 12, cap_raw=1 << 12, cap_pts=1 << 12)


def assert_same(got, want, label=""):
    for k in KEYS:
        assert np.array_equal(got[k], want[k]), (label, k, got[k].tolist(), want[k].tolist())
    assert rr.same_bits(got["path"], want["path"]), (label, "path")


def device_form(frx, vm, routes, pad, cap_window, cap_level, cap_raw, cap_pts, cap_total, stream=0, launch=None, repeat=1):
    """The outputs of the device form as route_batch_window_host lays them out; outputs and scratch are pre-filled with a sentinel and nothing is written
    behind either at the sizes the entry was given.  launch(call) runs the enqueueing call (default: directly), `repeat` times into the same buffers - the
    workspace is not touched in between, so every run finds the labels of the run before it."""
    off, pts = frx.pack_routes(routes)
    R, NL = len(routes), int(off[-1]) - len(routes)
    nbytes = frx.route_window_workspace(NL, cap_level, cap_raw, cap_pts, cap_window)
    host = dict(work=np.full(nbytes // 4 + PAD, ISENT, np.int32), path_off=np.full(R + 1 + PAD, ISENT, np.int32), path=np.full(3 * cap_total + PAD, SENTINEL),
                rst=np.full(R + PAD, ISENT, np.int32), lst=np.full(NL + PAD, ISENT, np.int32), lev=np.full(NL + PAD, ISENT, np.int32),
                mx=np.full(NL + PAD, ISENT, np.int32), win=np.full(8 * NL + PAD, ISENT, np.int32))
    bufs = {k: DevBuf(v) for k, v in host.items()}
    bufs.update(cells=DevBuf(vm.cells), off=DevBuf(off), pts=DevBuf(pts.reshape(-1)))
    try:
        ms = vm.device_struct(bufs["cells"].p)

        def call():
            frx.route_plan_window_batch_device(ms, R, NL, bufs["off"].p, bufs["pts"].p, pad, cap_window, cap_level, cap_raw, cap_pts, cap_total, bufs["work"].p,
                                               bufs["path_off"].p, bufs["path"].p, bufs["rst"].p, bufs["lst"].p, bufs["lev"].p, bufs["mx"].p, bufs["win"].p, stream)
        out = None
        for _ in range(repeat):
            (launch or (lambda f: f()))(call)
            g = {k: bufs[k].get(host[k]) for k in host}
            assert (g["work"][nbytes // 4:] == ISENT).all() and (g["path"][3 * cap_total:] == SENTINEL).all()
            for k, n in (("path_off", R + 1), ("rst", R), ("lst", NL), ("lev", NL), ("mx", NL), ("win", 8 * NL)):
                assert (g[k][n:] == ISENT).all(), k
            po = g["path_off"][:R + 1]
            assert po[0] == 0 and (np.diff(po) >= 1).all() and po[-1] <= cap_total and (g["path"][3 * po[-1]:] == SENTINEL).all()
            got = dict(path_off=po, path=g["path"][:3 * po[-1]].reshape(-1, 3), route_status=g["rst"][:R], leg_status=g["lst"][:NL], levels=g["lev"][:NL],
                       max_level_cells=g["mx"][:NL], leg_window=g["win"][:8 * NL].reshape(-1, 8))
            assert out is None or all(np.array_equal(out[k].view(np.uint8), got[k].view(np.uint8)) for k in got)   # run to run
            out = got
        return out
    finally:
        for d in bufs.values():
            d.close()


def three_forms(frx, vm, routes, pad, cap_window=None, label="", **caps):
    """host referee, blocking form and device form of one batch at the same capacities, compared; returns the referee's dict"""
    caps = {**BIG, **caps}
    cap_window = int(cap_window if cap_window is not None else vm.cells.size)
    want = vm.route_batch_window_host(routes, pad, cap_window, **caps)
    cap_total = caps.get("cap_total") or max(int(want["need"]), 2 * len(routes))
    caps["cap_total"] = cap_total
    want = vm.route_batch_window_host(routes, pad, cap_window, **caps)
    got = vm.route_batch_window(routes, pad, cap_window, **caps)
    assert_same(got, want, (label, "blocking"))
    assert got["need"] == want["need"] and got["fits"] == want["fits"], label
    assert_same(device_form(frx, vm, routes, pad, cap_window, caps["cap_level"], caps["cap_raw"], caps["cap_pts"], cap_total), want, (label, "device"))
    return want


def certified_legs_are_the_whole_map_legs(vm, routes, want):
    full = vm.route_batch_host(routes, **BIG)
    ok = want["leg_status"] == 0
    assert (full["leg_status"][ok] == 0).all() and np.array_equal(full["levels"][ok], want["levels"][ok])
    for r in np.flatnonzero(want["route_status"] == 0):
        assert rr.same_bits(want["paths"][r], full["paths"][r])
    return full


@pytest.fixture(scope="module")
def mixed(frx):
    dim = (20, 28, 5)
    rng = np.random.default_rng(17)
    cells = rr.box_map(rng, dim, 0.12)
    cells[(np.arange(cells.size) % 89) == 0] = -1                                                   # some unknown cells: crossed, refused as an end
    vm_origin = (-1.0, -1.4, 0.0)
    routes = [np.array([rr.centre(rr.free_cell(rng, cells, dim), vm_origin, RES, rng.uniform(-0.04, 0.04, 3)) for _ in range(int(rng.integers(2, 5)))]) for _ in range(38)]
    occ, unk = int(np.flatnonzero(cells == 100)[5]), int(np.flatnonzero(cells == -1)[2])
    cell = lambda i: [i % dim[0], i // dim[0] % dim[1], i // (dim[0] * dim[1])]                     # noqa: E731
    routes.append(np.array([routes[0][0], rr.centre(cell(occ), vm_origin, RES), routes[0][1]]))    # goal not free, then start not free
    routes.append(np.array([rr.centre(cell(unk), vm_origin, RES), routes[1][0]]))
    cells.setflags(write=False)
    return frx.VoxelMap(vm_origin, dim, RES, cells), routes


def test_a_mixed_batch_at_three_pads(frx, mixed):
    vm, routes = mixed
    seen = set()
    for pad in (0, 1, 3):
        want = three_forms(frx, vm, routes, pad, label=f"pad {pad}")
        certified_legs_are_the_whole_map_legs(vm, routes, want)
        seen |= set(int(s) for s in want["leg_status"])
        assert (want["leg_status"] == 0).sum() >= 30
        assert (want["leg_window"][want["leg_status"] == 1] == 0).all()
    assert {0, 1, 2, 7} <= seen


def test_windows_at_the_edges_of_the_label_words(frx):
    dim = (9, 11, 3)
    cells = np.zeros(int(np.prod(dim)), np.int8)
    cells[4 + 9 * 5 + 99 * 1] = 100                                                                 # one cell in the way of the straight column
    vm = frx.VoxelMap((0.0, 0.0, 0.0), dim, RES, cells)
    c = lambda *p: rr.centre(list(p), vm.origin, RES)                                              # noqa: E731
    # at pad 0 the window is the box of the two ends: x sizes 1, 2, 3 and 5 over 5 x 3 cells in y, z - 15, 30, 45 and 75 cells, none a multiple of 4 - and the
    # start is the box's last cell, so the last, partly used word is claimed; then one cell that is start and goal, in the middle and in the last cell of the map
    routes = [np.array([c(4 + k, 7, 2), c(4, 3, 0)]) for k in (0, 1, 2, 4)] + [np.array([c(2, 2, 1), c(2, 2, 1)]), np.array([c(8, 10, 2), c(8, 10, 2)])]
    want = three_forms(frx, vm, routes, 0, label="word edges")
    assert [int(v) for v in want["leg_window"][:4, 3]] == [1, 2, 3, 5] and all(int(n) % 4 for n in want["leg_window"][:4, 3:6].prod(axis=1))
    assert list(want["leg_window"][4]) == [2, 2, 1, 1, 1, 1, 0, 0] and list(want["leg_status"]) == [0] * 6
    assert [len(p) for p in want["paths"][4:]] == [1, 1]                                            # a whole route of one one-cell leg is one point
    certified_legs_are_the_whole_map_legs(vm, routes, want)
    three_forms(frx, vm, routes, 0, cap_window=75, label="word edges, cap_window exact")             # the label region is exactly the largest window
    three_forms(frx, vm, routes, 1, label="word edges, pad 1")


def test_a_level_wider_than_two_passes_of_the_workgroup(frx):
    dim = (40, 40, 3)
    vm = frx.VoxelMap((0.0, 0.0, 0.0), dim, RES, np.zeros(int(np.prod(dim)), np.int8))
    c = lambda *p: rr.centre(list(p), vm.origin, RES)                                              # noqa: E731
    routes = [np.array([c(0, 0, 1), c(39, 39, 1)]), np.array([c(13, 13, 1), c(26, 26, 1)])]
    want = three_forms(frx, vm, routes, 12, label="wide")
    assert list(want["leg_status"]) == [0, 0]
    assert int(want["leg_window"][0][6]) == -1 and int(want["leg_window"][1][6]) == 26 + 24        # the whole map, and a window open on four sides
    certified_legs_are_the_whole_map_legs(vm, routes, want)
    # three layers hold no level of more than 150 cells (a diagonal of the layer, three deep).  A level of more than 512 cells needs the third axis: the
    # shell of radius 12 around the goal, 4 x 144 + 2 cells less the one the map's top cuts off, inside a window of 32 x 25 x 24 at the same pad
    dim = (40, 40, 24)
    vm = frx.VoxelMap((0.0, 0.0, 0.0), dim, RES, np.zeros(int(np.prod(dim)), np.int8))
    routes = [np.array([c(33, 20, 12), c(20, 20, 12)])]
    want = three_forms(frx, vm, routes, 12, label="wide shell")
    assert list(want["leg_status"]) == [0] and int(want["levels"][0]) == 13 and int(want["max_level_cells"][0]) > 2 * THREADS, want["max_level_cells"]
    assert list(want["leg_window"][0]) == [8, 8, 0, 32, 25, 24, 13 + 24, 0]


def test_windows_clipped_at_a_corner_of_the_map(frx):
    dim = (20, 20, 4)
    grid = np.zeros(dim[::-1], np.int8)
    grid[:, 3, 1:9] = 100                                                                           # a wall across y = 3 that leaves x = 0 free
    vm = frx.VoxelMap((0.0, 0.0, 0.0), dim, RES, grid.reshape(-1))
    c = lambda *p: rr.centre(list(p), vm.origin, RES)                                              # noqa: E731
    routes = [np.array([c(2, 6, 1), c(2, 0, 1)]), np.array([c(3, 6, 1), c(3, 0, 1)]), np.array([c(0, 0, 0), c(1, 1, 0), c(0, 2, 3)])]
    want = three_forms(frx, vm, routes, 2, label="corner")
    # the first leg's window is clipped at x = 0, y = 0 and on both sides of z; its detour runs along the map's edge x = 0 and is as long as the limit
    assert list(want["leg_window"][0]) == [0, 0, 0, 5, 9, 4, 10, 0] and int(want["levels"][0]) == 10 and int(want["leg_status"][0]) == 0
    assert (want["paths"][0][:, 0] < RES).any()
    assert int(want["leg_status"][1]) == 7 and int(want["leg_window"][1][6]) == 10                 # one cell further from the edge: 12 steps against a limit of 10
    assert list(want["leg_status"][2:]) == [0, 0]
    certified_legs_are_the_whole_map_legs(vm, routes, want)


def test_the_certificate_on_its_edge(frx):
    k = 3
    dim = (14, 32, 3)
    grid = np.zeros(dim[::-1], np.int8)
    grid[:, 8, :] = 100; grid[:, 8, 6 + k] = 0                                                      # a gap k cells beside the straight line
    grid[:, 24, :] = 100; grid[:, 24, 6 + k + 1] = 0                                                # and one k + 1 cells beside it
    grid[:, 16, :] = 100                                                                            # nothing crosses from one half to the other
    vm = frx.VoxelMap((0.0, 0.0, 0.0), dim, RES, grid.reshape(-1))
    c = lambda *p: rr.centre(list(p), vm.origin, RES)                                              # noqa: E731
    routes = [np.array([c(6, 2, 1), c(6, 13, 1)]), np.array([c(6, 18, 1), c(6, 29, 1)])]            # D = M + 2 k and M + 2 (k + 1): pad = k and pad = k' - 1
    want = three_forms(frx, vm, routes, k, label="edge")
    assert list(want["leg_status"]) == [0, 7] and list(want["levels"]) == [11 + 2 * k, -1] and list(want["leg_window"][:, 6]) == [11 + 2 * k] * 2
    full = certified_legs_are_the_whole_map_legs(vm, routes, want)
    assert list(full["levels"]) == [11 + 2 * k, 11 + 2 * k + 2]
    assert list(three_forms(frx, vm, routes, k - 1, label="edge, below")["leg_status"]) == [7, 7]
    both = three_forms(frx, vm, routes, k + 1, label="edge, above")
    assert list(both["leg_status"]) == [0, 0] and rr.same_bits(both["path"], full["path"])


def test_every_status_at_its_exact_capacity(frx, mixed):
    vm, routes = mixed
    pad = 3
    full = three_forms(frx, vm, routes, pad, label="roomy")
    ok = full["leg_status"] == 0
    sizes = full["leg_window"][:, 3:6].astype(np.int64).prod(axis=1)

    def neighbours_stay(short, label):
        for r in np.flatnonzero(short["route_status"] == 0):
            assert rr.same_bits(short["paths"][r], full["paths"][r]), (label, r)
        assert np.array_equal(short["leg_window"], full["leg_window"]), label
    big = int(sizes.max())
    assert list(three_forms(frx, vm, routes, pad, cap_window=big, label="cap_window")["leg_status"]) == list(full["leg_status"])
    short = three_forms(frx, vm, routes, pad, cap_window=big - 1, label="cap_window one short")
    over = sizes == big
    assert (short["leg_status"][over] == 6).all() and (short["levels"][over] == -1).all() and (short["max_level_cells"][over] == 0).all()
    assert np.array_equal(short["leg_status"][~over], full["leg_status"][~over]) and 0 < over.sum() < len(over)
    neighbours_stay(short, "cap_window")
    for key, field, status in (("cap_level", "max_level_cells", 3), ("cap_raw", "levels", 4)):
        exact = int(full[field].max()) + (key == "cap_raw")
        same = three_forms(frx, vm, routes, pad, label=key, **{key: exact})
        assert list(same["leg_status"]) == list(full["leg_status"])
        short = three_forms(frx, vm, routes, pad, label=key + " one short", **{key: exact - 1})
        assert status in list(short["leg_status"]) and (short["leg_status"][~ok] != 0).all()
        neighbours_stay(short, key)
    # cap_pts counts a leg's own points
    first = np.concatenate([[0], np.cumsum([len(r) - 1 for r in routes])])
    leg_pts = []
    for r in np.flatnonzero(full["route_status"] == 0):
        for l in range(len(routes[r]) - 1):
            leg_pts.append(len(vm.route_batch_window_host([routes[r][l:l + 2]], pad, vm.cells.size, **BIG)["paths"][0]))
    exact = max(leg_pts)
    legs_of_whole = np.concatenate([np.arange(first[r], first[r + 1]) for r in np.flatnonzero(full["route_status"] == 0)])
    same = three_forms(frx, vm, routes, pad, label="cap_pts", cap_pts=exact)
    assert (same["leg_status"][legs_of_whole] == 0).all()
    short = three_forms(frx, vm, routes, pad, label="cap_pts one short", cap_pts=exact - 1)
    assert 5 in list(short["leg_status"][legs_of_whole])
    neighbours_stay(short, "cap_pts")


def test_on_a_callers_stream_twice_and_captured_in_a_graph(frx, mixed):
    """pure launches: three kernel nodes in a line; a replay gives the host's bits on a workspace that holds the labels of the run before"""
    vm, routes = mixed
    pad, cap_window = 3, int(vm.cells.size)
    want = vm.route_batch_window_host(routes, pad, cap_window, **BIG)
    cap_total = int(want["need"]) + 3
    H = hip()
    st = C.c_void_p()
    assert H.hipStreamCreate(C.byref(st)) == 0
    try:
        assert_same(device_form(frx, vm, routes, pad, cap_window, 1 << 12, 1 << 12, 1 << 12, cap_total, stream=st.value, repeat=2), want, "stream")
        graph, exe, n = C.c_void_p(), C.c_void_p(), C.c_size_t(0)
        try:
            def launch(call):
                assert H.hipStreamBeginCapture(st, 0) == 0                                         # hipStreamCaptureModeGlobal
                call()
                assert H.hipStreamEndCapture(st, C.byref(graph)) == 0
                assert H.hipGraphGetNodes(graph, None, C.byref(n)) == 0 and n.value == 3
                assert H.hipGraphInstantiate(C.byref(exe), graph, None, None, 0) == 0
                for _ in range(2):
                    assert H.hipGraphLaunch(exe, st) == 0 and H.hipStreamSynchronize(st) == 0
            assert_same(device_form(frx, vm, routes, pad, cap_window, 1 << 12, 1 << 12, 1 << 12, cap_total, stream=st.value, launch=launch), want, "graph")
        finally:
            if exe.value:
                H.hipGraphExecDestroy(exe)
            if graph.value:
                H.hipGraphDestroy(graph)
    finally:
        H.hipStreamDestroy(st)


def test_fallback_gives_the_whole_map_routes(frx, mixed):
    vm, routes = mixed
    full = vm.route_batch(routes, **BIG)
    for pad, cap_window in ((0, vm.cells.size), (3, 600)):
        plain = vm.route_batch_window(routes, pad, cap_window, **BIG)
        assert np.isin(plain["leg_status"], (6, 7)).any() and (cap_window != 600 or (plain["leg_status"] == 6).any())
        got = vm.route_batch_window(routes, pad, cap_window, fallback=True, **BIG)
        for k in ("path_off", "route_status", "levels"):
            assert np.array_equal(got[k], full[k]), (pad, k)
        assert (got["max_level_cells"] <= full["max_level_cells"]).all()                           # a certified leg built its levels inside its window
        assert rr.same_bits(got["path"], full["path"]) and all(rr.same_bits(a, b) for a, b in zip(got["paths"], full["paths"]))
        needed = np.isin(plain["leg_status"], (6, 7)) & (full["leg_status"] == 0)
        assert np.array_equal(got["leg_status"][needed], plain["leg_status"][needed]) and np.array_equal(got["leg_status"][~needed], full["leg_status"][~needed])
        assert np.array_equal(got["leg_window"], plain["leg_window"]) and got["need"] == full["need"] and got["fits"]
