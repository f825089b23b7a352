"""The route batch searched inside certified per-leg windows, on the host (frx_route_plan_levels_window_batch, frx_route_window_workspace;
csrc/frx_route_window_host.hpp) against the whole-map form (VoxelMap.route_batch_host): a leg is certified exactly when the whole-map leg exists and
is no longer than the window's limit (or the window is the whole map), a certified leg is the whole-map leg bit for bit, and a leg without a certificate says
7 in an open window and -1 in a whole-map one.  A wall with one gap puts the certificate on its edge; leg_window against the formula; the workspace against its
closed form; cap_window at its exact value; and the argument rules, all without a device."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import route_reference as rr  # noqa: E402

RES = 0.1
BIG = dict(cap_level=1 << 12, cap_raw=1 << 12, cap_pts=1 << 12)
K = 3                                                                                               # the gap's displacement in the wall map


def window_of(dim, s, g, pad):
    """leg_window's row by the formula: a side on the map's face is closed, every other side is open"""
    lo = [max(0, min(s[i], g[i]) - pad) for i in range(3)]
    hi = [min(dim[i] - 1, max(s[i], g[i]) + pad) for i in range(3)]
    is_open = any(lo[i] > 0 or hi[i] < dim[i] - 1 for i in range(3))
    m = sum(abs(s[i] - g[i]) for i in range(3))
    return lo + [hi[i] - lo[i] + 1 for i in range(3)] + [m + 2 * pad if is_open else -1, 0]


def random_map(rng):
    dim = (int(rng.integers(3, 15)), int(rng.integers(3, 15)), int(rng.integers(1, 6)))
    cells = np.where(rng.random(int(np.prod(dim))) < rng.uniform(0.10, 0.35), 100, 0).astype(np.int8)
    cells[rng.integers(0, cells.size, 4)] = 0                                                       # free cells exist
    return dim, cells


def wall_map(frx):
    """12 x 16 x 3, a wall across y = 8 on every layer with one gap at x = 6 + K: from (6, 2, 1) to (6, 13, 1) the shortest path holds M + 2 K steps"""
    dim = (12, 16, 3)
    grid = np.zeros(dim[::-1], np.int8)
    grid[:, 8, :] = 100
    grid[:, 8, 6 + K] = 0
    vm = frx.VoxelMap((0.0, 0.0, 0.0), dim, RES, grid.reshape(-1))
    route = np.array([rr.centre([6, 2, 1], vm.origin, RES), rr.centre([6, 13, 1], vm.origin, RES)])
    return vm, route


def test_random_maps_against_the_whole_map_search(frx):
    rng = np.random.default_rng(2024)
    n_legs = n_open_ok = n_refused = n_whole_window = n_whole_routes = 0
    for _ in range(160):
        dim, cells = random_map(rng)
        vm = frx.VoxelMap((0.0, 0.0, 0.0), dim, RES, cells)
        pad = int(rng.integers(0, 5))
        ends = [[rr.free_cell(rng, cells, dim) for _ in range(int(rng.integers(2, 5)))] for _ in range(3)]
        occ = np.flatnonzero(cells == 100)
        if len(occ):                                                                                # statuses 1 and 2: a gate inside an obstacle
            i = int(occ[0])
            ends.append([ends[0][0], [i % dim[0], i // dim[0] % dim[1], i // (dim[0] * dim[1])], ends[0][1]])
        routes = [np.array([rr.centre(c, vm.origin, RES, rng.uniform(-0.04, 0.04, 3)) for c in e]) for e in ends]
        full = vm.route_batch_host(routes, **BIG)
        win = vm.route_batch_window_host(routes, pad, cells.size, **BIG)
        assert win["fits"] and full["fits"]
        leg = 0
        for r, e in enumerate(ends):
            for l in range(len(e) - 1):
                fs, ws, row = int(full["leg_status"][leg]), int(win["leg_status"][leg]), [int(v) for v in win["leg_window"][leg]]
                if fs in (1, 2):
                    assert ws == fs and row == [0] * 8                                              # unchanged, and no window
                else:
                    assert row == window_of(dim, e[l], e[l + 1], pad), (dim, e[l], e[l + 1], pad, row)
                    limit = row[6]
                    certified = fs == 0 and (limit == -1 or int(full["levels"][leg]) <= limit)
                    assert (ws == 0) == certified, (fs, ws, limit, int(full["levels"][leg]))
                    if ws == 0:
                        assert int(win["levels"][leg]) == int(full["levels"][leg])
                        assert 1 <= int(win["max_level_cells"][leg]) <= int(full["max_level_cells"][leg])
                        n_open_ok += limit != -1
                    else:
                        assert ws == (-1 if limit == -1 else 7) and int(win["levels"][leg]) == -1
                        n_refused += ws == 7
                    if limit == -1:
                        assert ws == fs and int(win["max_level_cells"][leg]) == int(full["max_level_cells"][leg])
                        n_whole_window += 1
                n_legs += 1
                leg += 1
            if full["route_status"][r] == 0 and win["route_status"][r] == 0:
                assert np.array_equal(win["paths"][r], full["paths"][r]) and rr.same_bits(win["paths"][r], full["paths"][r])
                n_whole_routes += 1
            elif win["route_status"][r] != 0:
                assert rr.same_bits(win["paths"][r], routes[r][[0, -1]])                            # the placeholder
    # the mix: the test cannot pass by certifying nothing
    assert 4 * n_open_ok >= n_legs and n_refused >= 10 and n_whole_window >= 10 and n_whole_routes >= 40, (n_legs, n_open_ok, n_refused, n_whole_window, n_whole_routes)


def test_a_wall_with_one_gap_puts_the_certificate_on_its_edge(frx):
    vm, route = wall_map(frx)
    full = vm.route_batch_host([route], **BIG)
    m = 11
    assert list(full["leg_status"]) == [0] and int(full["levels"][0]) == m + 2 * K
    at = vm.route_batch_window_host([route], K, vm.cells.size, **BIG)
    assert list(at["leg_status"]) == [0] and int(at["levels"][0]) == m + 2 * K and int(at["leg_window"][0][6]) == m + 2 * K
    assert rr.same_bits(at["path"], full["path"]) and list(at["path_off"]) == list(full["path_off"])
    assert list(at["leg_window"][0]) == [6 - K, 0, 0, 2 * K + 1, 16, 3, m + 2 * K, 0]              # y and z reach the map's faces: x alone is open
    below = vm.route_batch_window_host([route], K - 1, vm.cells.size, **BIG)
    assert list(below["leg_status"]) == [7] and list(below["route_status"]) == [1] and int(below["levels"][0]) == -1
    assert int(below["leg_window"][0][6]) == m + 2 * (K - 1) and rr.same_bits(below["path"], route)


def test_leg_window_rows_and_the_workspace_formula(frx):
    dim = (30, 40, 8)
    vm = frx.VoxelMap((-1.5, -2.0, 0.0), dim, RES, np.zeros(int(np.prod(dim)), np.int8))
    pairs = [([0, 0, 0], [29, 39, 7]), ([0, 0, 0], [0, 0, 0]), ([29, 39, 7], [29, 39, 7]), ([10, 12, 3], [14, 20, 4]), ([2, 37, 0], [5, 30, 7]), ([1, 1, 1], [1, 1, 1])]
    routes = [np.array([rr.centre(a, vm.origin, RES), rr.centre(b, vm.origin, RES)]) for a, b in pairs]
    for pad in (0, 1, 3, 1 << 20):
        got = vm.route_batch_window_host(routes, pad, vm.cells.size, **BIG)
        assert (got["leg_status"] == 0).all()                                                       # an empty map: every straight box holds a shortest path
        for (a, b), row in zip(pairs, got["leg_window"]):
            assert [int(v) for v in row] == window_of(dim, a, b, pad), (a, b, pad)
        if pad == 1 << 20:
            assert (got["leg_window"][:, 6] == -1).all() and (got["leg_window"][:, 3:6] == dim).all()
    assert list(vm.route_batch_window_host(routes, 0, vm.cells.size, **BIG)["leg_window"][0]) == [0, 0, 0, 30, 40, 8, -1, 0]   # corner to corner at pad 0
    assert list(vm.route_batch_window_host(routes, 0, vm.cells.size, **BIG)["leg_window"][1]) == [0, 0, 0, 1, 1, 1, 0, 0]      # one cell: limit 0
    # the workspace: a closed form of its arguments, none of them the map
    legs, cl, cr, cp, cw = 7, 300, 90, 500, 70001
    up8 = lambda b: (b + 7) // 8 * 8                                                                # noqa: E731
    want = up8(up8(up8(24 * cp * legs) + 4 * legs) + 4 * (2 * cl + cr) * legs)
    want = up8(want + 4 * ((cw + 3) // 4) * legs)
    assert frx.route_window_workspace(legs, cl, cr, cp, cw) == want
    assert frx.route_window_workspace(1, 1, 1, 1, 69) == 24 + 8 + 16 + 4 * 18 == frx.route_search_workspace((23, 3, 1), 1, 1, 1, 1)
    per_leg = 24 * 4096 + 4 + 4 * (2 * 16384 + 4096) + 4 * ((1 << 20) // 4)
    assert abs(frx.route_window_workspace(2048, 16384, 4096, 4096, 1 << 20) - 2048 * per_leg) <= 32   # 2 048 legs in 2.6 GB whatever the map
    assert frx.route_window_workspace(1, 1, 1, 1, (1 << 31) - 4) == 24 + 8 + 16 + (1 << 31)                 # 2^31 - 4 label bytes, padded to 8
    for args in ((0, 1, 1, 1, 1), (1, 0, 1, 1, 1), (1, 1, 0, 1, 1), (1, 1, 1, 0, 1), (1, 1, 1, 1, 0), (1, 1, 1, 1, (1 << 31) - 3)):
        with pytest.raises(frx.FrxError) as e:
            frx.route_window_workspace(*args)
        assert e.value.code == -1, args
    with pytest.raises(frx.FrxError) as e:
        frx.route_window_workspace((1 << 31) - 1, (1 << 31) - 1, 1, (1 << 31) - 1, 1 << 20)
    assert e.value.code == -5


def test_cap_window_at_its_exact_value(frx):
    rng = np.random.default_rng(5)
    dim = (14, 14, 5)
    cells = rr.box_map(rng, dim, 0.05)
    vm = frx.VoxelMap((0.0, 0.0, 0.0), dim, RES, cells)
    ends = [[rr.free_cell(rng, cells, dim) for _ in range(n)] for n in (3, 2, 4, 2)]
    routes = [np.array([rr.centre(c, vm.origin, RES) for c in e]) for e in ends]
    pad = 1
    roomy = vm.route_batch_window_host(routes, pad, cells.size, **BIG)
    sizes = roomy["leg_window"][:, 3:6].astype(np.int64).prod(axis=1)
    assert (roomy["leg_status"] == 0).sum() >= 5 and len(set(sizes)) > 3
    big = int(sizes.max())
    same = vm.route_batch_window_host(routes, pad, big, **BIG)
    for k in ("path_off", "route_status", "leg_status", "levels", "max_level_cells", "leg_window"):
        assert np.array_equal(same[k], roomy[k]), k
    assert rr.same_bits(same["path"], roomy["path"])
    short = vm.route_batch_window_host(routes, pad, big - 1, **BIG)
    over = sizes > big - 1
    assert over.any() and not over.all()
    assert (short["leg_status"][over] == 6).all() and (short["levels"][over] == -1).all() and (short["max_level_cells"][over] == 0).all()
    assert np.array_equal(short["leg_status"][~over], roomy["leg_status"][~over]) and np.array_equal(short["levels"][~over], roomy["levels"][~over])
    assert np.array_equal(short["leg_window"], roomy["leg_window"])                                  # a refused window is still reported
    first = np.concatenate([[0], np.cumsum([len(e) - 1 for e in ends])])
    for r in range(len(routes)):
        if over[first[r]:first[r + 1]].any():
            assert short["route_status"][r] == 1 and rr.same_bits(short["paths"][r], routes[r][[0, -1]])
        else:
            assert short["route_status"][r] == roomy["route_status"][r] and rr.same_bits(short["paths"][r], roomy["paths"][r])   # the neighbours stay as they were


def test_argument_rules_without_a_device(frx):
    vm, route = wall_map(frx)
    routes = [route, route[::-1].copy()]
    L = frx.lib()
    off, pts = frx.pack_routes(routes)
    R, NL = 2, 2
    outs = [np.zeros(R + 1, np.int32), np.zeros((4096, 3)), np.zeros(R, np.int32), np.zeros(NL, np.int32), np.zeros(NL, np.int32), np.zeros(NL, np.int32),
            np.zeros((NL, 8), np.int32)]
    need = C.c_int()

    def call(entry, ms=vm._s, n_routes=R, off_=off, pts_=pts, pad=2, cap_window=4096, caps=(64, 64, 64, 4096), drop=None):
        o = [a.ctypes.data for a in outs] + [C.addressof(need)]
        if drop is not None:
            o[drop] = None
        head = (0,) if entry == "frx_route_plan_window_batch" else ()
        return getattr(L, entry)(*head, C.byref(ms) if ms is not None else None, n_routes, off_.ctypes.data if off_ is not None else None,
                                 pts_.ctypes.data if pts_ is not None else None, pad, cap_window, *caps, *o)

    assert call("frx_route_plan_levels_window_batch") == 0
    for entry in ("frx_route_plan_levels_window_batch", "frx_route_plan_window_batch"):
        assert call(entry, ms=None) == -1 and call(entry, off_=None) == -1 and call(entry, pts_=None) == -1
        for k in range(8):
            assert call(entry, drop=k) == -1, (entry, k)
        assert call(entry, n_routes=0) == -1
        for k in range(3):
            caps = [64, 64, 64, 4096]; caps[k] = 0
            assert call(entry, caps=tuple(caps)) == -1
        assert call(entry, caps=(64, 64, 64, 2 * R - 1)) == -1 and b"cap_total" in L.frx_last_error()
        assert call(entry, pad=-1) == -1 and b"pad" in L.frx_last_error()
        assert call(entry, pad=(1 << 20) + 1) == -1 and b"pad" in L.frx_last_error()
        assert call(entry, cap_window=0) == -1 and b"cap_window" in L.frx_last_error()
        assert call(entry, cap_window=(1 << 31) - 3) == -1 and b"cap_window" in L.frx_last_error()
        short = off.copy(); short[1] = 1
        assert call(entry, off_=short) == -1 and b"fewer than 2" in L.frx_last_error()
        for res, dim in ((0.0, vm.dim), (RES, (12, 0, 3)), (RES, (1 << 16, 1 << 16, 1))):
            bad = frx.VoxelMapStruct((C.c_double * 3)(0.0, 0.0, 0.0), (C.c_int * 3)(*[int(d) for d in dim]), res, vm.cells.ctypes.data)
            assert call(entry, ms=bad) == -1, (entry, res, dim)
    assert call("frx_route_plan_levels_window_batch", pad=1 << 20, cap_window=(1 << 31) - 4) == 0   # both bounds are inside
    ms = vm.device_struct(1 << 20)
    good = dict(n_routes=R, n_legs=NL, pt_off_dev=8, pts_dev=8, pad=2, cap_window=4096, cap_level=64, cap_raw=64, cap_pts=64, cap_total=4096, work_dev=8,
                path_off_dev=8, path_dev=8, route_status_dev=8, leg_status_dev=8, leg_levels_dev=8, leg_max_level_dev=8, leg_window_dev=8)
    for key, val in [(k, 0) for k in good if k.endswith("_dev")] + [("n_routes", 0), ("cap_level", 0), ("cap_raw", 0), ("cap_pts", 0), ("cap_total", 2 * R - 1),
                                                                    ("n_legs", R - 1), ("work_dev", 12), ("pad", -1), ("pad", (1 << 20) + 1), ("cap_window", 0),
                                                                    ("cap_window", (1 << 31) - 3)]:
        with pytest.raises(frx.FrxError) as e:
            frx.route_plan_window_batch_device(ms, **{**good, key: val})
        assert e.value.code == -1, key
    if L.frx_device_count() < 1:
        assert call("frx_route_plan_window_batch") == -2 and b"no HIP device" in L.frx_last_error()
        with pytest.raises(frx.FrxError) as e:
            frx.route_plan_window_batch_device(ms, **good)
        assert e.value.code == -2
    for name in ("frx_route_plan_levels_window_batch", "frx_route_window_workspace", "frx_route_plan_window_batch_device", "frx_route_plan_window_batch"):
        assert name in frx.ABI_SYMBOLS and hasattr(L, name)
