"""frx_corridor_generate_batch without a device: the scene builder's self-checks (tests/corridor_states.py), every argument error of the blocking form (reported
before a device is looked for) and the Python mirror's unpacking of a hand-written CSR."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import corridor_states as cs  # noqa: E402

INVALID_ARG = -1


def test_world_is_decision_safe_and_covers_the_cases(frx, sc):
    w = cs.world(frx, sc)                                                   # asserts the margins of every path, with and without the map
    n = [len(p) for p in w["paths"]]
    assert len(n) == 9 and n[1] == 2 and len(set(n)) >= 6                   # ragged, a 2-point path among them
    assert 400 <= len(w["cloud"]) <= 3000
    assert all(len(r) >= 1 for r in w["ref"]) and len(w["ref"][1]) == 1
    # the sight lines matter: some route gets another corridor with the map than without
    assert any(len(a) != len(b) or any(x.shape != y.shape for x, y in zip(a, b)) for a, b in zip(w["ref"], w["ref_free"]))
    # the blocked path: every step of it is blocked, so every segment is one step long; its cells are the local box, floor and ceiling
    fog = w["paths"][4]
    assert all(H.shape[1] == 8 for H in w["ref"][4]) and len(w["ref"][4]) >= 4 and len(fog) == 19


@pytest.mark.parametrize("seed,gates,n_obs", [(11, 1, 400), (12, 2, 1200)])
def test_small_scenes_are_decision_safe(frx, sc, seed, gates, n_obs):
    path, cloud, vm = cs.small_scene(frx, sc, seed, gates, n_obs)
    assert 30 <= len(path) <= 150 and len(cloud) == n_obs and (vm.cells == 100).sum() > 0


def test_dense_scene_puts_stop_and_exit_on_the_window_edges(frx):
    path, cloud = cs.dense_scene(frx)                                       # asserts the margins of all six cases
    for (ms, bx), lane in zip(cs.EDGE_CASES, (255, 256, 257, 255, 256, 257)):
        cells = frx.corridor_generate(path, cloud, np.array([bx, 4.0, 2.5]), cs.MAP_HEIGHT, max_seg=ms)
        d = np.linalg.norm(path - path[0], axis=1)
        stop = int(np.argmax(d >= ms))                                      # first point the length test stops at; the first window starts at point 1
        if bx == 4.005:
            assert stop - 1 == lane
        else:
            k = stop - 1
            H = cells[0][:, :-2]
            outside = (np.einsum("dk,ndk->nk", H[:3], path[:, :, None] - H[3:][None]) > 1e-10).any(axis=1)
            first = k + int(np.argmax(outside[k:]))
            assert outside[k:].any() and first - k == lane                  # the exit scan's windows start at point k


def test_clump_world_overflows_only_the_lone_path(frx, sc):
    lone, cloud = cs.clump_world(frx, sc)
    assert len(cloud) == len(cs.world(frx, sc)["cloud"]) + 5000
    box = frx.line_segment_dilate(lone[8], lone[12], cs.BBOX, np.zeros((0, 3)))[0]      # a box that holds the clump
    inside = (np.einsum("dk,ndk->nk", box[:3], cloud[:, :, None] - box[3:][None]) <= 1e-10).all(axis=1)
    assert inside.sum() > 4096


def test_sight_pairs_cover_both_verdicts_and_the_border(frx):
    vm = cs.sight_map(frx)
    pairs = cs.sight_pairs(vm)
    assert set(pairs) == {"span2", "span4", "span10", "span20", "leaving", "occupied_end", "random"}
    for name, (a, b) in pairs.items():
        v = np.array([vm.is_blocked(p, q) for p, q in zip(a, b)])
        assert v.any() and not v.all(), name
    # the 10-cell rays: a sample on a cell border to within rounding (the third of eleven: a + 2.5 res); the 2- and 4-cell rays keep clear of borders
    a, b = pairs["span10"]
    assert max(cs.border_samples(p, q) for p, q in zip(a, b)) < 1e-9
    a, b = pairs["span4"]
    assert min(cs.border_samples(p, q) for p, q in zip(a, b)) > 0.05


def _args(frx):
    """a valid call, as a dict of keyword -> value, whose entries the cases below spoil one at a time"""
    off = np.array([0, 3, 5], np.int32); path = np.arange(15, dtype=np.float64); obs = np.ones(6); bbox = np.array([4.0, 4.0, 2.5])
    cells = np.zeros(8, np.int8)
    m = frx.VoxelMapStruct((C.c_double * 3)(0, 0, 0), (C.c_int * 3)(2, 2, 2), 0.5, cells.ctypes.data)
    keep = dict(off=off, path=path, obs=obs, bbox=bbox, cells=cells, m=m, n_polys=np.zeros(2, np.int32), status=np.zeros(2, np.int32),
                h_off=np.zeros(2 * 4 + 1, np.int32), h_rec=np.zeros(6 * 64), n_rec=C.c_int())
    a = dict(device=0, n_paths=2, path_off=off.ctypes.data, path=path.ctypes.data, n_obs=2, obs=obs.ctypes.data, bbox=bbox.ctypes.data, map_height=3.0, max_seg=4.0,
             map=C.addressof(m), cap_polys=4, cap_planes=16, n_polys=keep["n_polys"].ctypes.data, status=keep["status"].ctypes.data, cap_rec=64,
             n_rec=C.addressof(keep["n_rec"]), h_off=keep["h_off"].ctypes.data, h_rec=keep["h_rec"].ctypes.data)
    return a, keep


def _call(frx, a):
    order = ("device", "n_paths", "path_off", "path", "n_obs", "obs", "bbox", "map_height", "max_seg", "map", "cap_polys", "cap_planes", "n_polys", "status",
             "cap_rec", "n_rec", "h_off", "h_rec")
    return frx.lib().frx_corridor_generate_batch(*[a[k] for k in order])


@pytest.mark.parametrize("field", ["path_off", "path", "obs", "bbox", "n_polys", "status", "n_rec", "h_off", "h_rec"])
def test_null_arguments_are_invalid(frx, field):
    a, keep = _args(frx)
    a[field] = None
    assert _call(frx, a) == INVALID_ARG and b"frx_corridor_generate_batch" in frx.lib().frx_last_error()


@pytest.mark.parametrize("case", ["n_paths", "short_path", "non_monotone", "cap_planes", "cap_planes_large", "max_seg_zero", "max_seg_nan", "cap_polys", "map_res",
                                  "map_dim", "map_cells"])
def test_out_of_range_arguments_are_invalid(frx, case):
    a, keep = _args(frx)
    if case == "n_paths": a["n_paths"] = 0
    if case == "short_path": keep["off"][:] = [0, 1, 5]
    if case == "non_monotone": keep["off"][:] = [0, 6, 5]
    if case == "cap_planes": a["cap_planes"] = 7
    if case == "cap_planes_large": a["cap_planes"] = 513
    if case == "max_seg_zero": a["max_seg"] = 0.0
    if case == "max_seg_nan": a["max_seg"] = float("nan")
    if case == "cap_polys": a["cap_polys"] = 0
    if case == "map_res": keep["m"].res = 0.0
    if case == "map_dim": keep["m"].dim[1] = 0
    if case == "map_cells": keep["m"].cells = None
    assert _call(frx, a) == INVALID_ARG


def test_valid_arguments_pass_the_argument_check(frx):
    """the same call unspoilt gets past the checks: no device -> FRX_ERR_NO_DEVICE, a device -> FRX_OK"""
    a, keep = _args(frx)
    keep["path"][:] = [0, 0, 1, 0, 1, 1, 0, 2, 1, 1, 0, 1, 1, 1, 1]
    keep["obs"][:] = [0.2, 0.2, 0.2, 0.7, 0.7, 0.7]
    rc = _call(frx, a)
    assert rc == (0 if frx.lib().frx_device_count() > 0 else -2)


def test_unpacking_a_hand_written_csr(frx):
    n_polys = np.array([2, 0, 1], np.int32)
    h_off = np.array([0, 3, 5, 9], np.int32)
    h_rec = np.arange(6 * 9, dtype=np.float64)
    got = frx.unpack_corridors(n_polys, h_off, h_rec)
    assert [len(g) for g in got] == [2, 0, 1]
    assert [H.shape for g in got for H in g] == [(6, 3), (6, 2), (6, 4)]
    assert np.array_equal(got[0][0][:, 1], np.arange(6, 12)) and np.array_equal(got[0][1][:, 0], np.arange(18, 24)) and np.array_equal(got[2][0][:, 3], np.arange(48, 54))
    assert got[0][0].flags["OWNDATA"] or got[0][0].base is not h_rec       # copies: the caller may reuse h_rec
