"""frx_route_plan_batch and frx_route_plan_batch_device against the host referee (VoxelMap.route_batch_host = frx_route_plan_levels_batch), bit for bit: every
point, offset, status, levels and max_level_cells.  The mixed batch of the CPU tests; levels wider than two workgroups and a dim[0] of 23; edges and sight
lines longer than one and than four wave-wide chunks (the sight line on a staircase, where the corner pass really walks it); every status at its exact capacity with the neighbours untouched; a caller's stream, twice, and a
captured graph replayed; and the hand-off of the device's CSR to frx_corridor_generate_batch_device."""
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
DIM, RES, ORIGIN = (24, 40, 6), 0.1, (-1.2, -2.0, 0.0)


def assert_same(got, want, label=""):
    for k in ("path_off", "route_status", "leg_status", "levels", "max_level_cells"):
        assert list(got[k]) == list(want[k]), (label, k, list(got[k]), list(want[k]))
    assert rr.same_bits(got["path"], want["path"]), (label, "path")
    assert got["need"] == want["need"] and got["fits"] == want["fits"], label


def device_form(frx, vm, routes, cap_level, cap_raw, cap_pts, cap_total, stream=0, launch=None, repeat=1, keep=None, packed=None, min_pts=2):
    """The outputs of the device form as route_batch_host lays them out; outputs and scratch are pre-filled with a sentinel and nothing is written behind either
    at the sizes the entry was given.  launch(call) runs the enqueueing call (default: directly), `repeat` times into the same buffers.  packed: (pt_off, pts)
    where the offsets are not frx.pack_routes' (they may begin above 0); min_pts: 1 where a whole route of one one-cell leg is one point."""
    off, pts = packed if packed is not None else frx.pack_routes(routes)
    R, NL = len(routes), int(off[-1]) - int(off[0]) - len(routes)
    nbytes = frx.route_search_workspace(vm.dim, NL, cap_level, cap_raw, cap_pts)
    host = dict(work=np.full(nbytes // 4 + PAD, ISENT, np.int32), path_off=np.full(R + 1 + PAD, ISENT, np.int32), path=np.full(3 * cap_total + PAD, SENTINEL),
                rst=np.full(R + PAD, ISENT, np.int32), lst=np.full(NL + PAD, ISENT, np.int32), lev=np.full(NL + PAD, ISENT, np.int32),
                mx=np.full(NL + PAD, ISENT, np.int32))
    bufs = {k: DevBuf(v) for k, v in host.items()}
    bufs.update(cells=DevBuf(vm.cells), off=DevBuf(off), pts=DevBuf(pts.reshape(-1)))
    try:
        ms = vm.device_struct(bufs["cells"].p)

        def call():
            frx.route_plan_batch_device(ms, R, NL, bufs["off"].p, bufs["pts"].p, cap_level, cap_raw, cap_pts, cap_total, bufs["work"].p, bufs["path_off"].p,
                                        bufs["path"].p, bufs["rst"].p, bufs["lst"].p, bufs["lev"].p, bufs["mx"].p, stream)
        out = None
        for _ in range(repeat):
            (launch or (lambda f: f()))(call)
            g = {k: bufs[k].get(host[k]) for k in host}
            assert (g["work"][nbytes // 4:] == ISENT).all() and (g["path"][3 * cap_total:] == SENTINEL).all()
            for k, n in (("path_off", R + 1), ("rst", R), ("lst", NL), ("lev", NL), ("mx", NL)):
                assert (g[k][n:] == ISENT).all(), k
            po = g["path_off"][:R + 1]
            assert po[0] == 0 and (np.diff(po) >= min_pts).all() and po[-1] <= cap_total and (g["path"][3 * po[-1]:] == SENTINEL).all()
            got = dict(path_off=po, path=g["path"][:3 * po[-1]].reshape(-1, 3), route_status=g["rst"][:R], leg_status=g["lst"][:NL], levels=g["lev"][:NL],
                       max_level_cells=g["mx"][:NL])
            assert out is None or all(np.array_equal(out[k].view(np.uint8), got[k].view(np.uint8)) for k in got)   # run to run
            out = got
        if keep is not None:
            keep(bufs, ms)
        return out
    finally:
        for d in bufs.values():
            d.close()


def both_forms(frx, vm, routes, label="", **caps):
    """host referee, blocking form and device form of one batch at the same capacities, compared; returns the referee's dict"""
    want = vm.route_batch_host(routes, **caps)
    cap_total = caps.get("cap_total") or max(int(want["need"]), 2 * len(routes))
    want = vm.route_batch_host(routes, **{**caps, "cap_total": cap_total})
    assert_same(vm.route_batch(routes, **{**caps, "cap_total": cap_total}), want, (label, "blocking"))
    d = device_form(frx, vm, routes, caps.get("cap_level", 1 << 12), caps.get("cap_raw", 1 << 12), caps.get("cap_pts", 1 << 12), cap_total)
    for k in d:
        if k == "path":
            assert rr.same_bits(d[k], want[k]), (label, k)
        else:
            assert list(d[k]) == list(want[k]), (label, k)
    return want


@pytest.fixture(scope="module")
def mixed(frx):
    cells, routes = rr.mixed_batch(DIM, ORIGIN, RES)
    cells.setflags(write=False)
    return frx.VoxelMap(ORIGIN, DIM, RES, cells), routes


def test_the_mixed_batch_of_the_cpu_tests(frx, mixed):
    vm, routes = mixed
    want = both_forms(frx, vm, routes, "mixed", cap_level=1 << 12, cap_raw=1 << 12, cap_pts=1 << 12)
    assert list(want["route_status"]) == rr.MIXED_ROUTE_STATUS
    assert {k: int(v) for k, v in enumerate(want["leg_status"]) if v != 0} == rr.MIXED_LEG_FAILURES   # unknown cells at a start and at a goal among them
    for r in (2, 5, 6, 7):
        assert rr.same_bits(want["paths"][r], routes[r][[0, -1]])                                    # the placeholder


def test_levels_wider_than_two_workgroups_and_an_odd_row_length(frx):
    rng = np.random.default_rng(3)
    for dim in ((48, 72, 10), (23, 31, 5)):
        cells = rr.box_map(rng, dim, 0.05)
        mid = [d // 2 for d in dim]
        cells[0] = cells[mid[0] + dim[0] * mid[1] + dim[0] * dim[1] * mid[2]] = 0                   # a far corner and the middle stay free
        vm = frx.VoxelMap((0.0, 0.0, 0.0), dim, RES, cells)
        routes = [np.array([rr.centre(rr.free_cell(rng, cells, dim), vm.origin, RES, rng.uniform(-0.04, 0.04, 3)) for _ in range(n)]) for n in (2, 3, 2)]
        far = [np.array([rr.centre([0, 0, 0], vm.origin, RES), rr.centre(mid, vm.origin, RES)])]    # levels around the middle: shells of an octahedron
        want = both_forms(frx, vm, routes + far, str(dim), cap_level=1 << 12, cap_raw=1 << 12, cap_pts=1 << 12)
        assert (want["leg_status"] == 0).any()
        if dim[0] == 48:
            assert want["max_level_cells"].max() > 2 * THREADS, want["max_level_cells"]


def test_edges_and_sight_lines_longer_than_the_chunks(frx):
    dim = (34, 300, 3)
    cells = np.zeros(int(np.prod(dim)), np.int8)
    vm = frx.VoxelMap((0.0, 0.0, 0.0), dim, RES, cells)
    c = lambda x, y, z: rr.centre([x, y, z], vm.origin, RES)                                       # noqa: E731
    routes = [np.array([c(2, 5, 1), c(2, 285, 1)]),                                                # one straight edge of 280 cells
              np.array([c(3, 290, 1), c(3, 260, 1), c(1, 100, 2)]),                                # 30 cells back, then a long diagonal
              np.array([c(3, 5, 1), c(30, 285, 1)])]                                               # a shallow diagonal of 280 cells: a staircase of corners
    want = both_forms(frx, vm, routes, "long", cap_level=1 << 10, cap_raw=1 << 10, cap_pts=1 << 11)
    assert (want["leg_status"] == 0).all()
    leg = want["paths"][0]
    assert (leg[:, 0] == leg[0, 0]).all() and (leg[:, 2] == leg[0, 2]).all()                        # straight along y: one edge after removeLinePts
    n_cells = len(leg) - 1
    assert n_cells * RES / 0.02 > 256                                                               # samples of that edge (its vertices are collinear: no long chord here)
    back = want["paths"][1][:31]
    assert (back[:, 0] == back[0, 0]).all() and 64 < 30 * RES / 0.02 <= 256
    # the staircase: at a corner the chord is strictly shorter, so the corner pass keeps its first vertex and walks the sight line to every later one.  The
    # restatement's simplified path, whose samples are the referee's bit for bit, is one edge, and that edge was walked as a chord of more than 256 samples
    om = rr.Map(vm.origin, dim, RES, cells)
    simple, samples = rr.simplified_path(om, routes[2][0], routes[2][1])
    assert rr.same_bits(samples, want["paths"][2])
    walks = [rr.walk_samples(om, a, b) for a, b in zip(simple[:-1], simple[1:])]
    assert len(simple) == 2 and max(walks) - 1 > 256, walks


def test_every_status_at_its_exact_capacity(frx):
    rng = np.random.default_rng(8)
    cells = rr.box_map(rng, DIM, 0.04).reshape(DIM[::-1]).copy()
    cells[:, 34, :] = 100                                                                          # a sealed wall: nothing crosses y = 34
    cells[:, 35:, :] = 0
    cells = cells.reshape(-1)
    hidden = [rr.free_cell(rng, cells, DIM) for _ in range(2)]
    while hidden[0][1] >= 34 or hidden[1][1] >= 34 or hidden[0] == hidden[1]:
        hidden = [rr.free_cell(rng, cells, DIM) for _ in range(2)]
    for h in hidden:
        cells[h[0] + DIM[0] * h[1] + DIM[0] * DIM[1] * h[2]] = -1                                    # two unknown cells: crossed by the search, refused as an end
    unknown = [rr.centre(h, ORIGIN, RES) for h in hidden]
    vm = frx.VoxelMap(ORIGIN, DIM, RES, cells)
    occ = int(np.flatnonzero(cells == 100)[7])
    inside = rr.centre([occ % DIM[0], occ // DIM[0] % DIM[1], occ // (DIM[0] * DIM[1])], ORIGIN, RES)

    def near():
        while True:
            cell = rr.free_cell(rng, cells, DIM)
            if cell[1] < 34:
                return rr.centre(cell, ORIGIN, RES, rng.uniform(-0.04, 0.04, 3))
    beyond = rr.centre([5, 37, 2], ORIGIN, RES)
    routes = [np.array([near(), near()]), np.array([near(), beyond]), np.array([near(), near(), near()]), np.array([inside, near()]), np.array([near(), inside]),
              np.array([near(), near()]), np.array([unknown[0], near()]), np.array([near(), unknown[1]])]
    big = dict(cap_level=1 << 12, cap_raw=1 << 12, cap_pts=1 << 12)
    full = both_forms(frx, vm, routes, "all statuses", **big)
    assert list(full["leg_status"]) == [0, -1, 0, 0, 1, 2, 0, 1, 2]
    for r in (1, 3, 4, 6, 7):
        assert rr.same_bits(full["paths"][r], routes[r][[0, -1]])                                    # the placeholder
    ok = full["leg_status"] == 0
    for key, field, status in (("cap_level", "max_level_cells", 3), ("cap_raw", "levels", 4)):
        exact = int(full[field].max()) + (key == "cap_raw")
        same = both_forms(frx, vm, routes, key, **{**big, key: exact})
        assert list(same["leg_status"]) == list(full["leg_status"])
        short = both_forms(frx, vm, routes, key + " one short", **{**big, key: exact - 1})
        assert status in list(short["leg_status"]) and (short["leg_status"][~ok] != 0).all()
        for r in np.flatnonzero(short["route_status"] == 0):
            assert rr.same_bits(short["paths"][r], full["paths"][r])                               # the neighbours stay as they were
    # cap_pts counts a leg's own points: route 2's legs share one point
    leg_pts = [len(full["paths"][0]), len(full["paths"][5])]
    two = vm.route_batch_host([routes[2][:2]], **big), vm.route_batch_host([routes[2][1:]], **big)
    exact = max(leg_pts + [len(t["paths"][0]) for t in two])
    same = both_forms(frx, vm, routes, "cap_pts", **{**big, "cap_pts": exact})
    assert list(same["leg_status"]) == list(full["leg_status"])
    short = both_forms(frx, vm, routes, "cap_pts one short", **{**big, "cap_pts": exact - 1})
    assert 5 in list(short["leg_status"])
    # cap_total one point short of the sum: the last whole route takes its placeholder
    total = int(full["path_off"][-1])
    short = both_forms(frx, vm, routes, "cap_total one short", **{**big, "cap_total": total - 1})
    assert list(short["route_status"]) == [0, 1, 0, 1, 1, 2, 1, 1] and not short["fits"] and short["need"] == total


def test_on_a_callers_stream_twice_and_captured_in_a_graph(frx, mixed):
    """pure launches: four kernel nodes in a line, and a replay gives the host's bits"""
    vm, routes = mixed
    want = vm.route_batch_host(routes, cap_level=1 << 12, cap_raw=1 << 12, cap_pts=1 << 12)
    cap_total = int(want["need"]) + 3
    H = hip()
    st = C.c_void_p()
    assert H.hipStreamCreate(C.byref(st)) == 0

    def check(got, label):
        for k in got:
            assert (rr.same_bits(got[k], want[k]) if k == "path" else list(got[k]) == list(want[k])), (label, k)
    try:
        check(device_form(frx, vm, routes, 1 << 12, 1 << 12, 1 << 12, cap_total, stream=st.value, repeat=2), "stream")
        graph, exe, n = C.c_void_p(), C.c_void_p(), C.c_size_t(0)
        try:
            def launch(call):
                assert H.hipStreamBeginCapture(st, 0) == 0                                         # hipStreamCaptureModeGlobal
                call()
                assert H.hipStreamEndCapture(st, C.byref(graph)) == 0
                assert H.hipGraphGetNodes(graph, None, C.byref(n)) == 0 and n.value == 4
                assert H.hipGraphInstantiate(C.byref(exe), graph, None, None, 0) == 0
                for _ in range(2):
                    assert H.hipGraphLaunch(exe, st) == 0 and H.hipStreamSynchronize(st) == 0
            check(device_form(frx, vm, routes, 1 << 12, 1 << 12, 1 << 12, cap_total, stream=st.value, launch=launch), "graph")
        finally:
            if exe.value:
                H.hipGraphExecDestroy(exe)
            if graph.value:
                H.hipGraphDestroy(graph)
    finally:
        H.hipStreamDestroy(st)


def test_the_csr_goes_straight_into_the_corridor_kernel(frx, mixed):
    vm, routes = mixed
    want = vm.route_batch_host(routes, cap_level=1 << 12, cap_raw=1 << 12, cap_pts=1 << 12)
    cap_total = int(want["need"])
    R, cap_polys, cap_planes = len(routes), 48, 96
    occ = np.argwhere(vm.cells.reshape(DIM[::-1]) == 100)[:, ::-1]
    cloud = np.ascontiguousarray((occ + 0.5) * RES + np.array(ORIGIN))
    bbox = np.array([1.0, 1.0, 0.5])
    sizes = dict(slot=R * cap_polys * cap_planes * 6, cp=R * cap_polys, npol=R, st=R)
    result = {}

    def corridors(path_off_dev, path_dev, ms):
        host = {k: (np.full(n, SENTINEL) if k == "slot" else np.full(n, ISENT, np.int32)) for k, n in sizes.items()}
        out = {k: DevBuf(v) for k, v in host.items()}
        cl = DevBuf(cloud.reshape(-1))
        try:
            frx.corridor_generate_batch_device(R, path_off_dev, path_dev, len(cloud), cl.p, bbox, DIM[2] * RES, 1.0, ms, cap_polys, cap_planes, out["slot"].p,
                                               out["cp"].p, out["npol"].p, out["st"].p, 0)
            return {k: out[k].get(host[k]) for k in host}
        finally:
            cl.close()
            for d in out.values():
                d.close()

    def keep(bufs, ms):
        result["device"] = corridors(bufs["path_off"].p, bufs["path"].p, ms)
        up_off, up_path = DevBuf(want["path_off"]), DevBuf(want["path"].reshape(-1))
        try:
            result["host"] = corridors(up_off.p, up_path.p, ms)
        finally:
            up_off.close(); up_path.close()
    device_form(frx, vm, routes, 1 << 12, 1 << 12, 1 << 12, cap_total, keep=keep)
    a, b = result["device"], result["host"]
    assert list(a["st"]) == list(b["st"]) and list(a["npol"]) == list(b["npol"]) and list(a["cp"]) == list(b["cp"])
    assert np.array_equal(a["slot"].view(np.uint64), b["slot"].view(np.uint64))
    assert (a["npol"][a["st"] == 0] >= 1).all() and (a["st"] == 0).any()
