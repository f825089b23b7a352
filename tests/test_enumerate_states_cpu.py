"""frx_enumerate_vertices_batch without a device: the numpy restatement (tests/enumerate_reference.py) equals the host's frx_enumerate_vertices bit for bit on
every state of tests/enumerate_states.py, the states have the edge properties their docstring claims (asserted from the restatement's ranks and keys), and the
three new entries report their argument errors before a device is looked for."""
import ctypes as C
import os
import sys
from collections import Counter

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import corridor_states as cs  # noqa: E402
import enumerate_reference as er  # noqa: E402
import enumerate_states as es  # noqa: E402

INVALID_ARG, NO_DEVICE = -1, -2


def corridor_polytopes(frx, sc, ids=(0, 3)):
    """every cell and every overlap of consecutive cells of the host corridors of the world's routes 0 and 2 (paths 0 and 3), as record arrays"""
    w = cs.world(frx, sc)
    out = []
    for i in ids:
        cells = [np.ascontiguousarray(H.T) for H in w["ref"][i]]
        for c, rec in enumerate(cells):
            out.append(rec)
            if c + 1 < len(cells):
                out.append(np.concatenate([rec, cells[c + 1]]))
    return out


def all_states(frx, sc):
    named = [("tetrahedron", es.tetrahedron()), ("cube", es.cube()), ("pyramid8", es.pyramid(8)), ("pyramid40", es.pyramid(40)), ("open_cube", es.open_cube()),
             ("two_cubes", es.two_cubes()), ("sphere13", es.sphere(13, es.SEED_13)), ("sphere12", es.sphere(12, es.SEED_12)), ("sphere62", es.sphere(62, es.SEED_62))]
    named += [(name, rec) for name, rec, _, _ in es.window_states(er.enumerate_ref)]
    named += [(f"corridor{i}", rec) for i, rec in enumerate(corridor_polytopes(frx, sc))]
    return named


def test_restatement_equals_the_host_bit_for_bit(frx, sc):
    n_ok = 0
    for name, rec in all_states(frx, sc):
        e = er.enumerate_ref(rec)
        nv, verts, verdict = er.host_enum(frx, rec)
        assert nv == len(e["vertices"]) and verdict == e["verdict"], (name, nv, len(e["vertices"]), verdict, e["verdict"])
        if verts is not None:
            assert np.array_equal(verts, e["vertices"]), name
            n_ok += 1
    assert n_ok >= 40                                                       # (the corridors alone give dozens of cells and overlaps)


def test_small_states_have_their_properties():
    assert er.enumerate_ref(es.tetrahedron())["verdict"] == er.POLY_OK and len(er.enumerate_ref(es.tetrahedron())["ranks"]) == 4
    cube = er.enumerate_ref(es.cube())
    keys = np.rint(cube["vertices"] / 1e-7).astype(np.int64)
    assert cube["verdict"] == er.POLY_OK and len(keys) == 8 and (keys < 0).any() and len(set(keys[:, 0])) == 2 and len(set(map(tuple, keys[:, :2]))) == 4
    assert [tuple(k) for k in keys] == sorted(tuple(k) for k in keys)
    open_ = er.enumerate_ref(es.open_cube())
    assert open_["verdict"] == er.POLY_UNBOUNDED and len(open_["vertices"]) == 4
    two = er.enumerate_ref(es.two_cubes())
    assert two["verdict"] == er.POLY_FLAT and len(two["vertices"]) == 4 and len(two["ranks"]) > 4       # duplicates among the 12 planes


@pytest.mark.parametrize("d", [8, 40])
def test_pyramid_apex_is_found_by_every_triple_of_side_planes(d):
    e = er.enumerate_ref(es.pyramid(d))
    assert e["verdict"] == er.POLY_OK and len(e["vertices"]) == d + 1
    keys = [tuple(k) for k in e["keys"]]
    apex, n = Counter(keys).most_common(1)[0]
    assert n == d * (d - 1) * (d - 2) // 6
    at = np.array([k == apex for k in keys])
    pts = e["points"][at]
    assert len(set(map(tuple, pts))) > 1                                    # the twins differ in their last bits
    first = int(e["ranks"][at][0])
    v = e["vertices"][sorted(set(keys)).index(apex)]
    assert np.array_equal(v, pts[0]) and first in e["owner"]                # the survivor is the first in triple order, with its own coordinates
    if d == 40:
        assert n == 9880 and len(set(int(r) // 256 for r in e["ranks"][at])) >= 39


def test_sphere_states():
    for K, seed in ((13, es.SEED_13), (12, es.SEED_12), (62, es.SEED_62)):
        e = er.enumerate_ref(es.sphere(K, seed))
        assert e["verdict"] == er.POLY_OK and len(e["ranks"]) == len(e["vertices"])             # one feasible triple per vertex
    assert len(er.enumerate_ref(es.sphere(62, es.SEED_62))["vertices"]) == 82
    assert 13 * 12 * 11 // 6 == 286 and 12 * 11 * 10 // 6 == 220


def test_window_states_put_a_vertex_on_the_named_rank():
    states = es.window_states(er.enumerate_ref)
    assert [r for _, rec, r, _ in states if len(rec) == 13] == [255, 256, 257, 63, 64, 65] and [r for _, rec, r, _ in states if len(rec) == 12] == [219, 0]
    for name, rec, r, key in states:
        e = er.enumerate_ref(rec)
        assert e["verdict"] == er.POLY_OK and r in e["ranks"], name
        assert tuple(e["keys"][list(e["ranks"]).index(r)]) == key, name    # the same vertex, now found by the triple of that rank
        assert er.rank_of(len(rec), *es.unrank(len(rec), r)) == r
    assert all(er.rank_of(9, *t) == i for i, t in enumerate(er.triples(9)))


# ---- arguments ----
def _batch_args():
    rec = np.concatenate([es.cube(), es.tetrahedron()])
    keep = dict(coarse_n=np.array([2], np.int32), h_off=np.array([0, 6, 10], np.int32), rec=rec, status=np.zeros(3, np.int32), v_off=np.zeros(4, np.int32),
                n_vert=C.c_int(), v_rec=np.zeros(3 * 64))
    a = dict(device=0, B=1, coarse_n=keep["coarse_n"].ctypes.data, h_off=keep["h_off"].ctypes.data, h_rec=rec.ctypes.data, cap_v=16, status=keep["status"].ctypes.data,
             v_off=keep["v_off"].ctypes.data, cap_vert=64, n_vert=C.addressof(keep["n_vert"]), v_rec=keep["v_rec"].ctypes.data)
    return a, keep


def _batch(frx, a):
    order = ("device", "B", "coarse_n", "h_off", "h_rec", "cap_v", "status", "v_off", "cap_vert", "n_vert", "v_rec")
    return frx.lib().frx_enumerate_vertices_batch(*[a[k] for k in order])


@pytest.mark.parametrize("case", ["coarse_n", "h_off", "h_rec", "status", "v_off", "n_vert", "v_rec", "B", "coarse_zero", "non_monotone", "cap_v_small", "cap_v_large"])
def test_blocking_form_refuses_bad_arguments(frx, case):
    a, keep = _batch_args()
    if case in a and case != "B": a[case] = None
    if case == "B": a["B"] = 0
    if case == "coarse_zero": keep["coarse_n"][0] = 0
    if case == "non_monotone": keep["h_off"][:] = [0, 11, 10]
    if case == "cap_v_small": a["cap_v"] = 3
    if case == "cap_v_large": a["cap_v"] = 513
    assert _batch(frx, a) == INVALID_ARG and b"frx_enumerate_vertices_batch" in frx.lib().frx_last_error()


@pytest.mark.parametrize("case", ["n_tasks", "tasks", "h_rec", "v_slot", "nv", "status", "cap_v_small", "cap_v_large"])
def test_device_form_refuses_bad_arguments(frx, case):
    a = dict(n_tasks=1, tasks=8, h_rec=8, cap_v=16, v_slot=8, nv=8, status=8)      # (never dereferenced: the checks come first)
    if case in ("tasks", "h_rec", "v_slot", "nv", "status"): a[case] = None
    if case == "n_tasks": a["n_tasks"] = 0
    if case == "cap_v_small": a["cap_v"] = 3
    if case == "cap_v_large": a["cap_v"] = 513
    rc = frx.lib().frx_enumerate_vertices_batch_device(a["n_tasks"], a["tasks"], a["h_rec"], a["cap_v"], a["v_slot"], a["nv"], a["status"], None)
    assert rc == INVALID_ARG and b"frx_enumerate_vertices_batch_device" in frx.lib().frx_last_error()


@pytest.mark.parametrize("case", ["n_paths", "cap_polys", "cap_planes", "cell_planes", "n_polys", "tasks", "too_many"])
def test_slots_to_tasks_refuses_bad_arguments(frx, case):
    a = dict(n_paths=1, cap_polys=4, cap_planes=16, cell_planes=8, n_polys=8, tasks=8)
    if case in ("cell_planes", "n_polys", "tasks"): a[case] = None
    if case in ("n_paths", "cap_polys", "cap_planes"): a[case] = 0
    if case == "too_many": a.update(n_paths=1 << 20, cap_polys=1 << 10, cap_planes=512)
    rc = frx.lib().frx_corridor_slots_to_tasks_device(a["n_paths"], a["cap_polys"], a["cap_planes"], a["cell_planes"], a["n_polys"], a["tasks"], None)
    assert rc == INVALID_ARG and b"frx_corridor_slots_to_tasks_device" in frx.lib().frx_last_error()


def test_valid_arguments_pass_the_argument_check(frx):
    """the same blocking call unspoilt gets past the checks: no device -> FRX_ERR_NO_DEVICE, a device -> FRX_OK with the cube, its overlap with the tetrahedron
    and the tetrahedron; and without a device the two device forms say so too"""
    a, keep = _batch_args()
    rc = _batch(frx, a)
    if frx.lib().frx_device_count() > 0:
        assert rc == 0 and keep["v_off"].tolist()[:2] == [0, 8] and keep["status"][0] == frx.HV_OK and keep["status"][2] == frx.HV_OK
    else:
        assert rc == NO_DEVICE
        assert frx.lib().frx_enumerate_vertices_batch_device(1, 8, 8, 16, 8, 8, 8, None) == NO_DEVICE
        assert frx.lib().frx_corridor_slots_to_tasks_device(1, 4, 16, 8, 8, 8, None) == NO_DEVICE


def test_python_names(frx):
    assert {"frx_enumerate_vertices_batch", "frx_enumerate_vertices_batch_device", "frx_corridor_slots_to_tasks_device"} <= set(frx.ABI_SYMBOLS)
    assert (frx.HV_OK, frx.HV_UNBOUNDED, frx.HV_FLAT, frx.HV_PLANES, frx.HV_VERTICES, frx.HV_NONFINITE, frx.HV_SKIPPED) == tuple(range(7)) and frx.HV_MAX_PLANES == 256
