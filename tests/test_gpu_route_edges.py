"""The crafted states of the route batch (tests/route_states.py) on the device: frx_route_plan_batch and frx_route_plan_batch_device against the host
referee frx_route_plan_levels_batch, bit for bit, twice into the same sentinel-filled buffers; the states with offsets the wrappers never pack through the C
entries; the routes only the device form takes (one waypoint: status 3 beside undisturbed neighbours; none: the whole batch refused, every output written) against
the batch without them; and the sample-chunk, one-cell and offset states once more through a captured graph, replayed twice.  tests/test_route_states_cpu.py
holds the referee to the Python restatement on the same states and asserts, from the restatement alone, that every state sits on its edge."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import route_reference as rr  # noqa: E402
import route_states as rs  # noqa: E402
from test_gpu_route_batch import assert_same, both_forms, device_form  # noqa: E402
from test_gpu_trajectory_sample import hip  # noqa: E402

pytestmark = pytest.mark.gpu

STATES = rs.all_states()
HOST = [s for s in STATES if not s.extra.get("device_only")]
DEVICE_ONLY = [s for s in STATES if s.extra.get("device_only")]
GRAPH = [s for s in STATES if s.extra.get("graph")]
NO_POINTS = 3                                                             # ROUTE_NO_POINTS of csrc/frx_route_host.hpp


def referee(frx, s):
    """(map, what the device must give, cap_total): the host referee on the routes it accepts, laid out over ALL routes of the state as frx.h defines the
    device form's answer for the ones it does not accept."""
    vm = frx.VoxelMap(s.origin, s.dim, s.res, s.cells)
    routes = rs.host_routes(s)
    if "lead" in s.extra:
        off, pts = rs.pack(s)
        rc, need = rs.c_batch(frx, vm, "frx_route_plan_levels_batch", off, pts, s.caps, 1 << 16)
        assert rc == 0
        cap_total = need["need"]
        rc, host = rs.c_batch(frx, vm, "frx_route_plan_levels_batch", off, pts, s.caps, cap_total)
        assert rc == 0
        return vm, host, cap_total
    host = vm.route_batch_host(routes, **s.caps)
    cap_total = s.caps.get("cap_total") or max(int(host["need"]), 2 * len(routes))
    host = vm.route_batch_host(routes, **{**s.caps, "cap_total": cap_total})
    if not s.extra.get("device_only"):
        return vm, host, cap_total
    # the device-only states: a route of one waypoint is status 3 with that waypoint twice; a route without one refuses the batch
    refused = s.extra["refused"]
    legs = len(host["leg_status"]) if not refused else sum(len(r) for r in s.routes) - len(s.routes)
    paths, rst, it = [], [], iter(range(len(routes)))
    for wp in s.routes:
        k = next(it) if len(wp) >= 2 else None
        if k is not None and not refused:
            paths.append(host["paths"][k]); rst.append(int(host["route_status"][k]))
        else:
            paths.append(np.array([wp[0], wp[-1]]) if len(wp) else np.zeros((2, 3))); rst.append(NO_POINTS)
    want = dict(path_off=np.cumsum([0] + [len(p) for p in paths]).astype(np.int32), path=np.concatenate(paths), route_status=np.array(rst, np.int32))
    if refused:
        want.update(leg_status=np.full(legs, -1, np.int32), levels=np.full(legs, -1, np.int32), max_level_cells=np.zeros(legs, np.int32))
    else:
        want.update({k: host[k] for k in ("leg_status", "levels", "max_level_cells")})
    # room to spare: were the batch not refused, a route spliced from another route's leg slot would come back whole, not hidden behind ROUTE_NO_ROOM
    return vm, want, cap_total + 2 * (len(s.routes) - len(routes)) + 256


def run_device(frx, s, vm, cap_total, **kw):
    packed = rs.pack(s) if ("lead" in s.extra or s.extra.get("device_only")) else None
    return device_form(frx, vm, s.routes, s.caps["cap_level"], s.caps["cap_raw"], s.caps["cap_pts"], cap_total, packed=packed,
                       min_pts=1 if s.extra.get("one_point") else 2, **kw)


def assert_device(got, want, label):
    for k in got:
        if k == "path":
            assert rr.same_bits(got[k], want[k]), (label, k, got[k].tolist(), np.asarray(want[k]).tolist())
        else:
            assert list(got[k]) == list(want[k]), (label, k, list(got[k]), list(want[k]))


@pytest.mark.parametrize("s", HOST, ids=[s.label for s in HOST])
def test_blocking_and_device_form_equal_the_referee_twice(frx, s):
    vm, want, cap_total = referee(frx, s)
    if "lead" in s.extra:
        off, pts = rs.pack(s)
        rc, blocking = rs.c_batch(frx, vm, "frx_route_plan_batch", off, pts, s.caps, cap_total)
        assert rc == 0
        assert_same(blocking, want, (s.label, "blocking"))
    elif s.extra.get("one_point"):                                        # both_forms holds every route to two points or more
        assert_same(vm.route_batch(s.routes, **{**s.caps, "cap_total": cap_total}), want, (s.label, "blocking"))
    else:
        both = both_forms(frx, vm, s.routes, s.label, **s.caps)
        assert rr.same_bits(both["path"], want["path"])
    assert_device(run_device(frx, s, vm, cap_total, repeat=2), want, s.label)


def test_the_neighbours_of_ends_outside_are_as_without_them(frx):
    s = next(s for s in STATES if "neighbours" in s.extra)
    vm, want, cap_total = referee(frx, s)
    got = run_device(frx, s, vm, cap_total)
    alone = device_form(frx, vm, s.extra["alone"], s.caps["cap_level"], s.caps["cap_raw"], s.caps["cap_pts"], cap_total)
    po, pa = got["path_off"], alone["path_off"]
    for k, r in s.extra["neighbours"].items():
        assert got["route_status"][r] == 0 and rr.same_bits(got["path"][po[r]:po[r + 1]], alone["path"][pa[k]:pa[k + 1]]), r
    bad = [r for r in range(len(s.routes)) if r not in s.extra["neighbours"].values()]
    assert sorted(int(v) for v in got["leg_status"] if v) == [rr.START] * len(bad) + [rr.GOAL] * len(bad)   # every end outside: status 1 or 2, never a cell
    assert all(got["route_status"][r] == 1 for r in bad)


@pytest.mark.parametrize("s", DEVICE_ONLY, ids=[s.label for s in DEVICE_ONLY])
def test_routes_only_the_device_form_takes(frx, s):
    """The acceptance rule of frx.h: no route comes back whole with points that are not its own, and no entry of an output is left unwritten (device_form
    pre-fills every output with a sentinel; `want` covers every entry)."""
    vm, want, cap_total = referee(frx, s)
    got = run_device(frx, s, vm, cap_total, repeat=2)
    for k in got:
        assert not (np.asarray(got[k]) == -7).any(), (s.label, k, "an entry was left unwritten")
    host = vm.route_batch_host(rs.host_routes(s), **s.caps)
    it = iter(range(len(host["paths"])))
    for r, wp in enumerate(s.routes):                                     # a whole route carries its own points
        k = next(it) if len(wp) >= 2 else None
        if got["route_status"][r] == 0:
            assert k is not None and rr.same_bits(got["path"][got["path_off"][r]:got["path_off"][r + 1]], host["paths"][k]), (s.label, r)
    assert_device(got, want, s.label)
    assert (got["route_status"] == NO_POINTS).sum() == (len(s.routes) if s.extra["refused"] else 3)


@pytest.mark.parametrize("s", GRAPH, ids=[s.label for s in GRAPH])
def test_through_a_captured_graph_replayed_twice(frx, s):
    vm, want, cap_total = referee(frx, s)
    H = hip()
    st, graph, exe, n = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_size_t(0)
    assert H.hipStreamCreate(C.byref(st)) == 0
    try:
        def launch(call):
            assert H.hipStreamBeginCapture(st, 0) == 0                                             # hipStreamCaptureModeGlobal
            call()
            assert H.hipStreamEndCapture(st, C.byref(graph)) == 0
            assert H.hipGraphGetNodes(graph, None, C.byref(n)) == 0 and n.value == 4                 # still four kernel nodes
            assert H.hipGraphInstantiate(C.byref(exe), graph, None, None, 0) == 0
            for _ in range(2):
                assert H.hipGraphLaunch(exe, st) == 0 and H.hipStreamSynchronize(st) == 0
        assert_device(run_device(frx, s, vm, cap_total, stream=st.value, launch=launch), want, (s.label, "graph"))
    finally:
        if exe.value:
            H.hipGraphExecDestroy(exe)
        if graph.value:
            H.hipGraphDestroy(graph)
        H.hipStreamDestroy(st)
