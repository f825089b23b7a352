"""frx_enumerate_vertices_batch without a device: the numpy restatement (tests/enumerate_reference.py) equals the host's frx_enumerate_vertices bit for bit on
every state of tests/enumerate_states.py, the states have the edge properties their docstring claims (asserted from the restatement's ranks and keys), and the
three new entries report their argument errors before a device is looked for.  The states above 64 planes and 256 vertices have the counts and properties
their docstring claims; the restatement is run on those of up to 131 planes and on two of 256, the host alone judges the others.  The unranking of the kernel
(frx_enumerate_rank.hpp) is run rank by rank against the nested loops as a sanitized program of its own."""
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


# ---- above 64 planes and 256 vertices ----
def ceiling_states_small():
    """the new states the restatement is run on: K <= 131"""
    named = [(f"sphere{K}", es.sphere(K, 1)) for K in es.CEILING_K if K <= 131]
    named += [("prism128", es.prism(128)), ("prism129", es.prism(129)), ("flat_late", es.flat_late()), ("open_late", es.open_late()), ("open_sides", es.open_sides())]
    return named


_ref = {}


def ref_of(name, rec):
    if name not in _ref:
        _ref[name] = er.enumerate_ref(rec)
    return _ref[name]


def test_restatement_equals_the_host_on_the_ceiling_states(frx):
    named = ceiling_states_small()
    assert [len(rec) for _, rec in named] == [63, 64, 65, 128, 129, 130, 131, 76, 69, 70]
    for name, rec in named + [("sphere256_tangent", es.sphere(256, 1, 0.0)), ("prism254", es.prism(254))]:      # (two K = 256 states: seconds and most of a gigabyte each)
        e = ref_of(name, rec) if len(rec) <= 131 else er.enumerate_ref(rec)
        nv, verts, verdict = er.host_enum(frx, rec)
        assert nv == len(e["vertices"]) and verdict == e["verdict"], (name, nv, len(e["vertices"]), verdict, e["verdict"])
        if verts is not None:
            assert np.array_equal(verts, e["vertices"]), name
        else:
            assert name in ("flat_late", "open_late", "open_sides")
        if name == "sphere256_tangent":
            assert nv == 508 and len(e["ranks"]) == 508 and len(set(map(tuple, e["keys"]))) == 508        # one feasible triple per vertex


def test_plane_count_states(frx):
    assert es.CEILING_K == (63, 64, 65, 128, 129, 192, 193, 255, 256)
    got = [er.host_enum(frx, es.sphere(K, 1)) for K in es.CEILING_K]
    assert [g[2] for g in got] == [er.POLY_OK] * 9 and [g[0] for g in got] == [68, 76, 76, 106, 106, 136, 122, 140, 142] == list(es.CEILING_NV)
    for seed in (1, 2, 3):
        rec = es.sphere(256, seed, spread=0.0)
        nv, verts, verdict = er.host_enum(frx, rec)
        assert len(rec) == 256 and verdict == er.POLY_OK and nv == 508 == 2 * 256 - 4
        assert len(set(map(tuple, np.rint(verts / 1e-7).astype(np.int64)))) == 508


def test_prism_states(frx):
    for d, K, nv_want in ((128, 130, 256), (129, 131, 258), (254, 256, 508)):
        rec = es.prism(d)
        nv, verts, verdict = er.host_enum(frx, rec)
        assert len(rec) == K and verdict == er.POLY_OK and nv == nv_want == 2 * d
    # even d: opposite sides are antiparallel - triples of them fall to the determinant, pairs of them to the cross product
    pl = er.planes(es.prism(128))
    keep, _, _, _ = er.solve(pl, np.array([[0, 64, 128], [0, 64, 129], [1, 65, 3]]))
    assert not keep.any()
    u = np.cross(pl[:64, :3], pl[64:128, :3])
    assert (np.sqrt((u * u).sum(axis=1)) <= 1e-10).all()
    e = ref_of("prism128", es.prism(128))
    assert len(e["ranks"]) == 256 and e["verdict"] == er.POLY_OK                               # one feasible triple per vertex: (side i, side i + 1, cap)


@pytest.mark.parametrize("d", [254, 255])
def test_ceiling_pyramids(frx, d):
    rec = es.pyramid(d)
    nv, verts, verdict = er.host_enum(frx, rec)
    assert len(rec) == d + 1 and verdict == er.POLY_OK and nv == d + 1
    assert 255 * 254 * 253 // 6 == 2731135 and -(-2731135 // 256) == 10669                    # C(255, 3) triples of side planes, in that many windows of 256 ranks
    first = er.triple_point(rec, 0, 1, 2)                                   # the apex as the first triple in rank order finds it
    keys = np.rint(verts / 1e-7).astype(np.int64)
    at = np.nonzero((keys == np.rint(first / 1e-7).astype(np.int64)).all(axis=1))[0]
    assert len(at) == 1 and np.array_equal(verts[at[0]], first)
    other = er.triple_point(rec, 3, d // 2, d - 1)
    assert np.array_equal(np.rint(other / 1e-7), np.rint(first / 1e-7)) and not np.array_equal(other, first)      # a twin of the same key with other last bits


def test_verdicts_decided_beyond_the_first_wave(frx):
    flat = ref_of("flat_late", es.flat_late())
    assert len(es.flat_late()) == 76 and flat["verdict"] == er.POLY_FLAT and len(flat["vertices"]) == 4
    assert er.host_enum(frx, es.flat_late())[::2] == (4, er.POLY_FLAT)
    tight = np.nonzero(flat["slacks"] <= 1e-9)[0]
    assert len(tight) > 0 and tight.min() >= 64 and flat["slacks"][:64].min() > 1.0          # no plane of the first wave is without slack
    open_ = ref_of("open_late", es.open_late())
    rec = es.open_late()
    assert len(rec) == 69 and (rec[:64, 2] > 0).all() and (np.hypot(rec[:64, 0], rec[:64, 1]) > 0).all()
    assert open_["verdict"] == er.POLY_UNBOUNDED and open_["spans"] and er.host_enum(frx, rec)[2] == er.POLY_UNBOUNDED
    assert len(open_["ray_pairs"]) > 0 and open_["ray_pairs"].min() >= 256                   # the first trip of the pair loop finds no free ray
    sides = ref_of("open_sides", es.open_sides())
    assert len(es.open_sides()) == 70 and sides["verdict"] == er.POLY_UNBOUNDED and not sides["spans"] and len(sides["vertices"]) == 0
    assert er.host_enum(frx, es.open_sides())[::2] == (0, er.POLY_UNBOUNDED)


def test_unranking_against_the_nested_loops(tmp_path):
    """fast-racing_amd/csrc/frx_enumerate_rank.hpp (what k_enumerate unranks with) as a program of its own under the address and undefined-behaviour sanitizers:
    tests/hostcheck/enumerate_rank_main.cpp, every rank of every K in 3 ... 96 and around 128, 192 and 256"""
    import math
    import re
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("no g++: the host check cannot be built")
    exe = str(tmp_path / "enumerate_rank_san")
    src = os.path.join(root, "tests", "hostcheck", "enumerate_rank_main.cpp")
    b = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe, src],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert b.returncode == 0, b.stdout[-3000:]
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr.strip(), (r.stdout[-1000:], r.stderr[-3000:])
    m = re.search(r"(\d+) triples, (\d+) pairs, (\d+) disagreements", r.stdout)
    assert m, r.stdout
    Ks = list(range(3, 97)) + [127, 128, 129, 191, 192, 193, 255, 256]
    assert sum(math.comb(K, 3) for K in Ks) == 13467781 and sum(math.comb(K, 2) for K in Ks) == 291858
    assert (int(m.group(1)), int(m.group(2)), int(m.group(3))) == (13467781, 291858, 0)
    big = re.search(r"largest intermediate (\d+)", r.stdout)
    assert big and int(big.group(1)) == 256 * 255 * 254 < 2 ** 31             # n (n - 1) (n - 2) at n = 256, before the division


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
