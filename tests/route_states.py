"""Crafted states for the route batch (frx_route_plan_batch[_device], csrc/frx_route_kernel.hpp) - test infrastructure, not a test module.

A state is (label, origin, dim, res, cells, routes, caps) plus `check`, a function that asserts ON THE CPU, FROM THE PYTHON RESTATEMENT ALONE (route_reference.py,
oracle/jps_oracle.py) that the state really sits on the edge it is named for, and `extra`, what a test needs to know to run it:
  graph        run once more through a captured graph
  lead         the waypoint offsets begin at this value, with that many unused waypoints in front (only the C entries take such offsets)
  device_only  the batch holds routes of fewer than two waypoints, which only the device form accepts; refused = True when the device refuses the whole batch
The kernels' constants restated here: a wave is 64 lanes (one chunk of a sight line or of an edge's samples), a workgroup 256 (the stride of the splice plan over
routes), and k_route_clear strides over the labels above 8192 workgroups of 256 lanes and 8 bytes."""
from typing import Callable, NamedTuple

import numpy as np

import route_reference as rr

WAVE = 64
THREADS = 256
CLEAR_DIRECT_BYTES = 8192 * THREADS * 8                                   # above this k_route_clear strides


class State(NamedTuple):
    label: str
    origin: tuple
    dim: tuple
    res: float
    cells: np.ndarray
    routes: list
    caps: dict
    check: Callable
    extra: dict


def omap(s):
    return rr.Map(s.origin, s.dim, s.res, s.cells)


def host_routes(s):
    """the routes the host form accepts: at least two waypoints"""
    return [r for r in s.routes if len(r) >= 2]


def legs_of(routes):
    return [(r, a, b) for r, wp in enumerate(routes) for a, b in zip(wp[:-1], wp[1:])]


def _free(dim):
    return np.zeros(int(np.prod(dim)), np.int8)


def _wp(cells_xyz, origin, res, jitter=None):
    return np.array([rr.centre(c, origin, res, jitter[i] if jitter is not None else (0.0, 0.0, 0.0)) for i, c in enumerate(cells_xyz)], dtype=np.float64).reshape(-1, 3)


# ---- sample chunks: straight free edges whose sample counts sit on the ends of the 64-sample chunks of route_sample_pass ----
# (res, cells of the edge, samples as the restatement counts them with the accumulated d += 0.02).  0.1 x 12 is the accumulation's own edge: 60 additions of 0.02
# give 1.2000000000000004, one unit in the last place above the edge's length, so the edge has 60 samples, not 61.
SAMPLE_EDGES = ((0.1, 12, 60), (0.11, 11, 61), (0.14, 9, 63), (0.16, 8, 64), (0.1, 13, 65), (0.1, 51, 256), (0.1, 64, 321))


def _samples_state(res, n, count):
    dim, origin = (n + 2, n + 2, n + 2), (0.0, 0.0, 0.0)
    route = _wp([(1, 1, 1), (1 + n, 1, 1), (1 + n, 1 + n, 1), (1 + n, 1 + n, 1 + n)], origin, res)   # along x, then y, then z: the emit across edge ends

    def check(s):
        m = omap(s)
        for _, a, b in legs_of(s.routes):
            L = rr.leg_log(m, a, b)
            assert len(L["path"]) == 2, len(L["path"])                                             # one straight edge after removeLinePts
            assert rr.edge_samples(L["path"][0], L["path"][1]) == count, (res, n, rr.edge_samples(L["path"][0], L["path"][1]))
            assert len(L["samples"]) == n + 1                                                        # cap_pts is exact
    return State(f"samples: {count} on an edge of {n} cells at res {res}", origin, dim, res, _free(dim), [route],
                 dict(cap_level=1 << 13, cap_raw=n + 1, cap_pts=n + 1), check, dict(graph=True))


# ---- sight-line chunks: shallow staircases, where the corner pass keeps its first vertex and walks a chord to every later one ----
def _sight_state():
    origin, dim, res = (-1.2, 0.0, 0.0), (72, 30, 1), 0.1
    cells = _free(dim)
    # three bands of ten rows: (first cell along x, rise, the single cell of 100)
    bands = ((0, 3, (10, 3)), (1, 4, (11, 13)), (0, 7, (6, 23)))
    routes = []
    for k, (sx, h, occ) in enumerate(bands):
        cells[occ[0] + dim[0] * occ[1]] = 100
        routes.append(_wp([(sx, 10 * k + 2, 0), (sx + 62, 10 * k + 2 + h, 0)], origin, res))

    def check(s):
        m = omap(s)
        chords = [c for _, a, b in legs_of(s.routes) for c in rr.leg_log(m, a, b)["chords"]]
        walked = {md - 1 for _, _, md, _ in chords}
        assert {WAVE - 1, WAVE, WAVE + 1} <= walked, sorted(walked)                                   # walks of 63, 64 and 65 samples
        hits = sorted({hit for _, _, _, hit in chords if hit is not None})
        assert WAVE in hits, hits                                                                    # the last lane of the first chunk
        assert WAVE + 1 in hits, hits                                                                # lane 0 of the second chunk
        assert any(WAVE + 1 < h <= 2 * WAVE for h in hits), hits                                     # a whole chunk clear, blocked inside the next
        # no sample of any walk leaves the map: between two cell centres of the map it cannot, so the `out` ballot of route_blocked is unreachable
        for a, b, md, _ in chords:
            for n in range(1, md):
                assert not m.outside(m.float_to_int([a[i] + (b[i] - a[i]) * (1.0 / md) * n for i in range(3)]))
    return State("sight lines: first blocked sample 64, 65 and in the second chunk", origin, dim, res, cells, routes,
                 dict(cap_level=256, cap_raw=128, cap_pts=128), check, {})


# ---- cell values: an end must be == 0, the search crosses <= 0, a sight line is blocked by >= 100 ----
VALUES = (-128, -1, 0, 1, 50, 99, 100, 127)


def _values_state():
    origin, dim, res = (0.0, 0.0, 0.0), (16, 12, 1), 0.1
    g = np.zeros((dim[1], dim[0]), np.int8)
    g[:, 4] = -128                                                        # two full columns the search must cross
    g[:, 5] = -1
    soft = {50: (10, 6), 99: (10, 9)}                                     # the search goes around, the chord is cut across
    hard = {100: (10, 2), 127: (13, 6)}                                   # the search goes around and the chord stays blocked
    for v, (x, y) in {**soft, **hard}.items():
        g[y, x] = v
    g[11, 15] = 1
    cells = g.reshape(-1)
    cell = lambda x, y: (x, y, 0)                                                                    # noqa: E731
    routes = [_wp([cell(1, 2), cell(8, 2)], origin, res), _wp([cell(8, 10), cell(0, 0)], origin, res)]   # across the negative columns, both ways
    around = {}
    for v, (x, y) in {**soft, **hard}.items():
        around[v] = len(routes)
        routes.append(_wp([cell(x - 1, y), cell(x + 1, y)], origin, res))
    ends = {-128: (4, 3), -1: (5, 7), 1: (15, 11), **soft, **hard}
    on_value = {}
    for v, (x, y) in ends.items():                                        # a gate on the value: the leg into it fails at its goal, the leg out of it at its start
        on_value[v] = len(routes)
        routes.append(_wp([cell(7, 4), cell(x, y), cell(8, 8)], origin, res))

    def check(s):
        m = omap(s)
        assert set(VALUES) <= set(int(v) for v in np.unique(s.cells))
        ref = rr.route_batch(m, s.routes, **s.caps)
        assert list(ref["route_status"][:2]) == [0, 0]
        for r in (0, 1):                                                                             # the route really crosses both negative columns
            crossed = {int(s.cells[m.index(m.float_to_int(p))]) for p in ref["paths"][r]}
            assert {-128, -1} <= crossed, crossed
        for v in soft:                                                                               # around in the search, across in the result
            a, b = s.routes[around[v]]
            L = rr.leg_log(m, a, b)
            assert all(s.cells[m.index(m.float_to_int(p))] == 0 for p in L["raw"]) and len(L["raw"]) == 5
            assert any(s.cells[m.index(m.float_to_int(p))] == v for p in L["samples"]), v
            assert ref["route_status"][around[v]] == 0
        for v in hard:                                                                               # a chord blocked by exactly this value
            a, b = s.routes[around[v]]
            L = rr.leg_log(m, a, b)
            stopped = {int(s.cells[m.index(m.float_to_int([p[i] + (q[i] - p[i]) * (1.0 / md) * hit for i in range(3)]))]) for p, q, md, hit in L["chords"]
                       if hit is not None}
            assert stopped == {v}, (v, stopped)
            assert all(s.cells[m.index(m.float_to_int(p))] == 0 for p in L["samples"])
        first = sum(len(r) - 1 for r in s.routes[:on_value[-128]])
        for k, v in enumerate(ends):                                                                 # only 0 passes as an end
            assert list(ref["leg_status"][first + 2 * k:first + 2 * k + 2]) == [rr.GOAL, rr.START], v
    return State("cell values: -128, -1, 0, 1, 50, 99, 100, 127 under the three predicates", origin, dim, res, cells, routes,
                 dict(cap_level=64, cap_raw=64, cap_pts=64), check, {})


# ---- ends outside the map ----
def outside_points(origin, dim, res):
    """(what, point) with one coordinate outside the map, the other two at the centre of cell (1, 1, 1)"""
    inside = rr.centre((1, 1, 1), origin, res)
    out = []
    for axis in range(3):
        def at(v, axis=axis):
            p = list(inside); p[axis] = v
            return p
        out.append((f"one cell below the low face on axis {axis}", at(rr.centre((-1, -1, -1), origin, res)[axis])))
        out.append((f"one cell beyond the high face on axis {axis}", at(rr.centre(dim, origin, res)[axis])))
        for v in (1e6, -1e6, 1e300, -1e300, np.inf, -np.inf, np.nan):
            out.append((f"{v} on axis {axis}", at(v)))
    return out


def _outside_state():
    origin, dim, res = (-0.3, -0.2, 0.1), (6, 5, 4), 0.1
    good = [_wp([(1, 1, 1), (4, 3, 2)], origin, res), _wp([(5, 0, 3), (0, 4, 0), (2, 2, 2)], origin, res), _wp([(0, 0, 0), (5, 4, 3)], origin, res)]
    bad = outside_points(origin, dim, res)
    # beyond dim - 1 on x with a flat index x + dim[0] * y + ... that still falls inside the array: the cell (dim[0], 1, 1) would alias (0, 2, 1)
    bad.append(("beyond the last cell of a row", rr.centre((dim[0], 1, 1), origin, res)))
    a, b = rr.centre((2, 1, 1), origin, res), rr.centre((3, 3, 2), origin, res)
    routes, where = [good[0]], {0: 0}
    for k, (_, p) in enumerate(bad):                                      # a gate outside: the leg into it fails at its goal, the leg out of it at its start
        routes.append(np.array([a, p, b], dtype=np.float64))
        if k == len(bad) // 2:
            where[1] = len(routes); routes.append(good[1])
    where[2] = len(routes); routes.append(good[2])

    def check(s):
        m = omap(s)
        for what, p in bad:
            assert rr.end_cell(m, p) is None, what
        wrap = m.float_to_int(bad[-1][1])
        assert wrap[0] == s.dim[0] and 0 <= m.index(wrap) < s.cells.size                             # outside, at an index inside the array
        ref = rr.route_batch(m, s.routes, **s.caps)
        assert (ref["route_status"] == 0).sum() == 3 and sorted(int(v) for v in ref["leg_status"] if v) == [rr.START] * len(bad) + [rr.GOAL] * len(bad)
        alone = rr.route_batch(m, good, **s.caps)                                                    # the neighbours are as in the batch without the bad ends
        for k, r in where.items():
            assert rr.same_bits(ref["paths"][r], alone["paths"][k]) and len(alone["paths"][k]) > 2
    return State("ends outside: each face, far, infinite, not a number, and an aliasing index", origin, dim, res, _free(dim), routes,
                 dict(cap_level=64, cap_raw=32, cap_pts=32), check, dict(neighbours=where, alone=good))


# ---- start and goal of a leg in one cell ----
def _one_cell_states():
    origin, dim, res = (0.0, -0.3, 0.0), (6, 6, 2), 0.1
    p, q, r = (2, 3, 1), (5, 0, 0), (0, 5, 1)
    j = [(0.03, -0.04, 0.01), (-0.04, 0.02, -0.03), (0.0, 0.04, 0.04), (-0.02, -0.02, 0.0)]       # four points of one cell
    routes = [_wp([p, p], origin, res, j),                                # the only leg: a route of one point
              _wp([p, p, q], origin, res, j),                             # the first leg
              _wp([q, p, p, r], origin, res, [j[0], j[1], j[2], j[3]]),   # a middle leg
              _wp([q, p, p], origin, res, j),                             # the last leg
              _wp([p, p, p, p], origin, res, j)]                          # every leg: three legs, one point
    one_cell = [0, 1, 4, 7, 8, 9, 10]                                     # the legs with start and goal in one cell, in batch order

    def check_with(tiny):
        def check(s):
            m = omap(s)
            ref = rr.route_batch(m, s.routes, **s.caps)
            assert [k for k, L in enumerate(ref["levels"]) if L == 0] == one_cell and len(ref["levels"]) == 11
            for k, (_, a, b) in enumerate(legs_of(s.routes)):
                assert (m.float_to_int(a) == m.float_to_int(b)) == (k in one_cell) and (k not in one_cell or list(a) != list(b))
            assert len(ref["paths"][0]) == 1 and len(ref["paths"][4]) == 1 and list(ref["route_status"][[0, 4]]) == [0, 0]
            if tiny:                                                                                 # cap_raw = cap_pts = 1: only the one-cell legs pass
                assert [int(v) for v in ref["leg_status"]] == [0 if k in one_cell else rr.CAP_RAW for k in range(11)]
                assert list(ref["route_status"]) == [0, 1, 1, 1, 0]
            else:
                assert (ref["leg_status"] == 0).all() and (ref["route_status"] == 0).all()
                lens = [len(x) for x in ref["paths"]]
                assert lens[1] == lens[3] and lens[1] > 2 and lens[2] > lens[1]                      # take = 0 at the front, in the middle and at the back
        return check
    free = _free(dim)
    return [State("one-cell legs: only, first, middle, last and all", origin, dim, res, free, routes, dict(cap_level=64, cap_raw=32, cap_pts=32), check_with(False),
                  dict(graph=True, one_point=True)),
            State("one-cell legs at cap_raw = cap_pts = 1", origin, dim, res, free, routes, dict(cap_level=64, cap_raw=1, cap_pts=1), check_with(True),
                  dict(graph=True, one_point=True))]


# ---- the smallest capacities and degenerate maps ----
def _corridor_state(axis, n=9):
    dim = [1, 1, 1]; dim[axis] = n
    dim = tuple(dim)
    origin, res = (0.2, -0.1, 0.0), 0.1

    def cell(k):
        c = [0, 0, 0]; c[axis] = k
        return tuple(c)
    routes = [_wp([cell(0), cell(n - 1)], origin, res), _wp([cell(n - 1), cell(0)], origin, res),   # goal at an end: every level is one cell
              _wp([cell(0), cell(n // 2)], origin, res)]                                          # goal in the middle: level 1 holds two

    def check(s):
        ref = rr.route_batch(omap(s), s.routes, **s.caps)
        assert s.caps["cap_level"] == 1 and [int(v) for v in ref["leg_status"]] == [0, 0, rr.CAP_LEVEL]
        assert list(ref["max_level_cells"]) == [1, 1, 2] and list(ref["levels"][:2]) == [n - 1, n - 1]
        assert len(ref["paths"][0]) == n == s.caps["cap_raw"] == s.caps["cap_pts"]
    return State(f"corridor of {n} cells along axis {axis} at cap_level = 1", origin, dim, res, _free(dim), routes, dict(cap_level=1, cap_raw=n, cap_pts=n), check, {})


def _single_cell_state():
    origin, dim, res = (1.0, 2.0, 3.0), (1, 1, 1), 0.25
    routes = [_wp([(0, 0, 0), (0, 0, 0)], origin, res, [(0.1, -0.1, 0.05), (-0.12, 0.0, 0.1)])]

    def check(s):
        ref = rr.route_batch(omap(s), s.routes, **s.caps)
        assert list(ref["leg_status"]) == [0] and list(ref["levels"]) == [0] and len(ref["paths"][0]) == 1
    return State("a map of one cell at every capacity 1", origin, dim, res, _free(dim), routes, dict(cap_level=1, cap_raw=1, cap_pts=1, cap_total=2), check,
                 dict(one_point=True))


def _last_cell_state(dim):
    origin, res = (0.0, 0.0, 0.0), 0.1
    last = tuple(d - 1 for d in dim)
    routes = [_wp([(0, 0, 0), last], origin, res), _wp([last, (0, 0, 0), (dim[0] - 1, 0, dim[2] - 1)], origin, res)]

    def check(s):
        m = omap(s)
        n = int(np.prod(s.dim))
        assert n % 4 != 0 and m.index(last) == n - 1                                                 # the last label word is padded, and a leg claims its byte
        ref = rr.route_batch(m, s.routes, **s.caps)
        assert (ref["leg_status"] == 0).all() and list(ref["levels"][:2]) == [sum(last), sum(last)]
    return State(f"{dim}: a cell count not divisible by 4 and legs that label the last cell", origin, dim, res, _free(dim), routes,
                 dict(cap_level=64, cap_raw=32, cap_pts=32), check, {})


def _serpentine_state():
    origin, dim, res = (0.0, 0.0, 0.0), (16, 16, 1), 0.1
    g = np.zeros((16, 16), np.int8)
    for y in range(1, 16, 2):                                             # walls on the odd rows, open at alternating ends
        g[y, :] = 100
        g[y, 15 if (y // 2) % 2 == 0 else 0] = 0
    routes = [_wp([(0, 0, 0), (0, 14, 0)], origin, res), _wp([(0, 14, 0), (0, 0, 0)], origin, res),   # from end to end: every level one cell
              _wp([(0, 0, 0), (3, 14, 0)], origin, res)]                                          # a goal inside the last row: levels of two cells

    def check(s):
        ref = rr.route_batch(omap(s), s.routes, **s.caps)
        assert (ref["leg_status"] == 0).all() and ref["levels"].min() >= 120, ref["levels"]
        assert sorted(set(ref["max_level_cells"])) == [1, 2] and s.caps["cap_level"] == 2 and s.caps["cap_raw"] == ref["levels"].max() + 1 and s.caps["cap_pts"] == max(len(x) for x in ref["paths"])
    return State("a serpentine of more than 120 levels, one or two cells wide", origin, dim, res, g.reshape(-1), routes, dict(cap_level=2, cap_raw=135, cap_pts=133),
                 check, {})


# ---- offsets ----
MIXED = dict(dim=(24, 40, 6), res=0.1, origin=(-1.2, -2.0, 0.0))


def _mixed():
    cells, routes = rr.mixed_batch(MIXED["dim"], MIXED["origin"], MIXED["res"])
    return cells, routes


def _offset_states():
    cells, routes = _mixed()
    caps = dict(cap_level=1 << 12, cap_raw=1 << 12, cap_pts=1 << 12)
    args = (MIXED["origin"], MIXED["dim"], MIXED["res"], cells)

    def check_lead(s):
        ref = rr.route_batch(omap(s), s.routes, **s.caps)
        assert s.extra["lead"] == 3 and list(ref["route_status"]) == rr.MIXED_ROUTE_STATUS

    one = lambda k: np.array([routes[k][0]])                                                        # noqa: E731
    short = [one(3)] + routes[:4] + [one(0)] + routes[4:] + [one(7)]      # a route of one waypoint first, in the middle and last

    def check_short(s):
        assert [k for k, r in enumerate(s.routes) if len(r) == 1] == [0, 5, len(s.routes) - 1]
        assert sum(len(r) - 1 for r in s.routes) >= len(s.routes) and len(host_routes(s)) == len(routes)   # n_legs >= n_routes still holds
    empty = [routes[1][:3], np.zeros((0, 3)), routes[4][:3]]               # offsets 0, 3, 3, 6

    def check_empty(s):
        off = np.cumsum([0] + [len(r) for r in s.routes])
        assert list(off) == [0, 3, 3, 6] and off[-1] - len(s.routes) >= len(s.routes)               # three leg slots pass the check, four legs exist
        first = [int(off[r] - off[0] - r) for r in range(len(s.routes))]
        assert first == [0, 2, 1]                                                                    # not monotone: route 2's first slot is route 0's second leg
    return [State("offsets: the mixed batch behind three unused waypoints", *args, routes, caps, check_lead, dict(lead=3, graph=True)),
            State("offsets: routes of one waypoint first, in the middle and last", *args, short, caps, check_short, dict(device_only=True, refused=False, graph=True)),
            State("offsets: a route without a waypoint in the middle", *args, empty, caps, check_empty, dict(device_only=True, refused=True, graph=True))]


# ---- many routes: the splice plan strides over routes by a workgroup ----
def _many_states():
    origin, dim, res = (0.0, 0.0, 0.0), (8, 8, 2), 0.1
    rng = np.random.default_rng(17)
    cells = np.where(rng.random(int(np.prod(dim))) < 0.12, 100, 0).astype(np.int8)
    cells[rng.integers(0, cells.size, 4)] = -1
    pick = lambda: rr.centre([int(rng.integers(0, d)) for d in dim], origin, res, rng.uniform(-0.04, 0.04, 3))   # noqa: E731
    routes = [np.array([pick() for _ in range(int(rng.integers(2, 6)))]) for _ in range(300)]      # any cell: some ends are occupied or unknown
    caps = dict(cap_level=64, cap_raw=32, cap_pts=48)
    need = rr.route_batch(rr.Map(origin, dim, res, cells), routes, **caps)["need"]

    def check_with(short):
        def check(s):
            ref = rr.route_batch(omap(s), s.routes, **s.caps)
            assert len(s.routes) == 300 > THREADS and {len(r) for r in s.routes} == {2, 3, 4, 5}
            assert 30 < (ref["route_status"] == 0).sum() and (ref["route_status"] == 1).sum() > 30
            assert ref["route_status"][THREADS:].tolist().count(0) > 3                               # whole routes behind the first stride
            if short:
                assert s.caps["cap_total"] == ref["need"] - 1 and list(ref["route_status"]).count(rr.NO_ROOM) == 1
            else:
                assert rr.NO_ROOM not in list(ref["route_status"])
        return check
    return [State("many routes: 300 on a small map, some failing", origin, dim, res, cells, routes, caps, check_with(False), {}),
            State("many routes: cap_total one point short", origin, dim, res, cells, routes, {**caps, "cap_total": need - 1}, check_with(True), {})]


# ---- large clear: more label bytes than k_route_clear covers with one cell per lane ----
def _clear_state():
    origin, dim, res = (0.0, 0.0, 0.0), (64, 64, 64), 0.1
    rng = np.random.default_rng(23)
    routes = []
    for _ in range(72):
        a = [int(rng.integers(3, 61)) for _ in range(3)]
        axes = rng.permutation(3)[:int(rng.integers(2, 4))]                # two or three cells away, one step on each of as many axes
        step = [int(rng.choice((-1, 1))) if i in axes else 0 for i in range(3)]
        routes.append(_wp([a, [a[i] + step[i] for i in range(3)]], origin, res))

    def check(s):
        legs = sum(len(r) - 1 for r in s.routes)
        assert 4 * ((int(np.prod(s.dim)) + 3) // 4) * legs > CLEAR_DIRECT_BYTES                      # the label region: the clear must stride
        ref = rr.route_batch(omap(s), s.routes, **s.caps)
        assert (ref["leg_status"] == 0).all() and sorted(set(ref["levels"])) == [2, 3] and ref["max_level_cells"].max() <= s.caps["cap_level"]
    return State("large clear: 72 legs on a free 64^3 map", origin, dim, res, _free(dim), routes, dict(cap_level=64, cap_raw=8, cap_pts=8), check, {})


def pack(s):
    """(pt_off int32, pts float64 [.., 3]) of a state: packed from 0, or behind `lead` unused waypoints with offsets that begin at `lead`"""
    lead = int(s.extra.get("lead", 0))
    off = np.zeros(len(s.routes) + 1, np.int32)
    off[1:] = np.cumsum([len(r) for r in s.routes])
    pts = np.concatenate([np.full((lead, 3), 1.0e3)] + [np.asarray(r, dtype=np.float64).reshape(-1, 3) for r in s.routes])
    return off + lead, np.ascontiguousarray(pts)


def c_batch(frx, vm, entry, off, pts, caps, cap_total):
    """A host-pointer C entry of the route batch (frx_route_plan_levels_batch, or frx_route_plan_batch on device 0) on explicit offsets, which the Python
    wrappers never pass: (return code, the dict VoxelMap.route_batch_host gives)."""
    import ctypes as C
    R, NL = len(off) - 1, int(off[-1]) - int(off[0]) - (len(off) - 1)
    path_off = np.full(R + 1, -7, np.int32); path = np.full((cap_total, 3), -7.0); rst = np.full(R, -7, np.int32)
    lst, lev, mx = (np.full(max(NL, 1), -7, np.int32) for _ in range(3))
    need = C.c_int(-7)
    head = (0,) if entry == "frx_route_plan_batch" else ()
    rc = getattr(frx.lib(), entry)(*head, C.byref(vm._s), R, off.ctypes.data, pts.ctypes.data, int(caps["cap_level"]), int(caps["cap_raw"]), int(caps["cap_pts"]),
                                   int(cap_total), path_off.ctypes.data, path.ctypes.data, rst.ctypes.data, lst.ctypes.data, lev.ctypes.data, mx.ctypes.data,
                                   C.addressof(need))
    end = max(int(path_off[-1]), 0)
    return rc, dict(path_off=path_off, path=path[:end].copy(), paths=[path[path_off[r]:path_off[r + 1]].copy() for r in range(R)], route_status=rst,
                    leg_status=lst[:NL], levels=lev[:NL], max_level_cells=mx[:NL], need=need.value, fits=rc == 0)


_STATES = None


def all_states():
    global _STATES
    if _STATES is None:
        out = [_samples_state(*e) for e in SAMPLE_EDGES]
        out += [_sight_state(), _values_state(), _outside_state()] + _one_cell_states()
        out += [_corridor_state(axis) for axis in range(3)] + [_single_cell_state(), _last_cell_state((7, 9, 3)), _last_cell_state((5, 5, 5)), _serpentine_state()]
        out += _offset_states() + _many_states() + [_clear_state()]
        for s in out:
            s.cells.setflags(write=False)
        _STATES = out
    return _STATES


def labels():
    return [s.label for s in all_states()]
