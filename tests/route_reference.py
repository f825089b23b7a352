"""A Python restatement of the canonical level search of the route batch (csrc/frx_route_host.hpp) and of what follows it, for the tests.

Levels: numpy, whole level by whole level, on an array of integer levels (the library keeps 1 + level mod 3 in a byte).  Descent: the face neighbour one level
down whose squared cell distance to the goal is smallest, ties in the order -x, -y, -z, +z, +y, +x.  The tail is the oracle's restatement of the reference's
removeCornerPts, removeLinePts and samplePath (oracle/jps_oracle.py), the splice is frx_route_plan's: the shared point once.  An end of a leg becomes a cell by
route_end_cell's rule (end_cell).  For the crafted states (route_states.py): the samples of an edge as samplePath's accumulated d counts them (edge_samples), and
a log of every chord the corner passes walk, with its max_diff and its first blocked sample (leg_log)."""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle.jps_oracle import Map, c_round, remove_corner_pts, remove_line_pts, sample_path  # noqa: E402

STEPS = ((-1, 0, 0), (0, -1, 0), (0, 0, -1), (0, 0, 1), (0, 1, 0), (1, 0, 0))
OK, START, GOAL, NO_PATH, CAP_LEVEL, CAP_RAW, CAP_PTS = 0, 1, 2, -1, 3, 4, 5
WHOLE, LEG_FAILED, NO_ROOM = 0, 1, 2


def level_search(cells, dim, start, goal, cap_level=None, cap_raw=None):
    """(status, path start-first as a list of (x, y, z) or [], levels, max_level_cells) on cells (x fastest, <= 0 traversable)."""
    nx, ny, nz = (int(d) for d in dim)
    free = (np.asarray(cells).reshape(nz, ny, nx) <= 0)
    lev = np.full((nz, ny, nx), -1, np.int64)
    s = tuple(int(v) for v in start); g = tuple(int(v) for v in goal)
    lev[g[2], g[1], g[0]] = 0
    front = np.array([[g[0], g[1], g[2]]], np.int64)
    level, max_cells = 0, 1
    while lev[s[2], s[1], s[0]] < 0:
        cand = np.concatenate([front + np.array(st, np.int64) for st in STEPS])
        ok = (cand[:, 0] >= 0) & (cand[:, 0] < nx) & (cand[:, 1] >= 0) & (cand[:, 1] < ny) & (cand[:, 2] >= 0) & (cand[:, 2] < nz)
        cand = cand[ok]
        cand = cand[free[cand[:, 2], cand[:, 1], cand[:, 0]] & (lev[cand[:, 2], cand[:, 1], cand[:, 0]] < 0)]
        cand = np.unique(cand, axis=0) if len(cand) else cand
        max_cells = max(max_cells, len(cand))
        if cap_level is not None and len(cand) > cap_level:
            return CAP_LEVEL, [], -1, max_cells
        level += 1
        lev[cand[:, 2], cand[:, 1], cand[:, 0]] = level
        if lev[s[2], s[1], s[0]] >= 0:
            break
        if len(cand) == 0:
            return NO_PATH, [], -1, max_cells
        front = cand
    if cap_raw is not None and level + 1 > cap_raw:
        return CAP_RAW, [], level, max_cells
    path = [s]
    c = s
    for L in range(level, 0, -1):
        best, best_d = None, None
        for st in STEPS:
            n = (c[0] + st[0], c[1] + st[1], c[2] + st[2])
            if not (0 <= n[0] < nx and 0 <= n[1] < ny and 0 <= n[2] < nz) or lev[n[2], n[1], n[0]] != L - 1:
                continue
            d = (n[0] - g[0]) ** 2 + (n[1] - g[1]) ** 2 + (n[2] - g[2]) ** 2
            if best is None or d < best_d:
                best, best_d = n, d
        c = best
        path.append(c)
    return OK, path, level, max_cells


def end_cell(m: Map, p):
    """route_end_cell of csrc/frx_route_host.hpp: the cell of a leg's end, or None for an end outside the map.  The verdict is taken on the rounded quotient
    as a number, never on a converted int: beyond the map, infinite and not a number are outside.  Inside the map the cell is Map.float_to_int's."""
    c = []
    for i in range(3):
        q = (p[i] - m.origin[i]) / m.res - 0.5
        if not math.isfinite(q):
            return None
        r = c_round(q)                                                                             # a Python integer: no range to leave
        if r < 0 or r >= m.dim[i]:
            return None
        c.append(r)
    return c


def plan_leg(m: Map, start, goal, cap_level=None, cap_raw=None, cap_pts=None):
    """(status, sample points as an (n, 3) array, levels, max_level_cells) of one leg: plan_leg_levels of frx_search.cpp on the level search."""
    s = end_cell(m, start)
    if s is None or not m.is_free(s):
        return START, np.zeros((0, 3)), -1, 0
    g = end_cell(m, goal)
    if g is None or not m.is_free(g):
        return GOAL, np.zeros((0, 3)), -1, 0
    st, cells, levels, mx = level_search(m.cells, m.dim, s, g, cap_level, cap_raw)
    if st != OK:
        return st, np.zeros((0, 3)), levels, mx
    raw = [m.int_to_float(c) for c in cells]
    q = remove_corner_pts(m, raw)
    q = remove_corner_pts(m, q[::-1])[::-1]
    pts = np.array(sample_path(m, remove_line_pts(q)), dtype=np.float64).reshape(-1, 3)
    if cap_pts is not None and len(pts) > cap_pts:
        return CAP_PTS, np.zeros((0, 3)), levels, mx
    return OK, pts, levels, mx


def route_batch(m: Map, routes, cap_level=None, cap_raw=None, cap_pts=None, cap_total=None):
    """dict(paths, route_status, leg_status, levels, max_level_cells, need) of a list of waypoint arrays, as VoxelMap.route_batch_host reports them."""
    paths, rst, lst, lev, mx = [], [], [], [], []
    used = need = 0
    for r, wp in enumerate(routes):
        wp = np.asarray(wp, dtype=np.float64).reshape(-1, 3)
        out, whole = [], True
        for a, b in zip(wp[:-1], wp[1:]):
            st, pts, L, M = plan_leg(m, a, b, cap_level, cap_raw, cap_pts)
            lst.append(st); lev.append(L); mx.append(M)
            if st != OK:
                whole = False
                continue
            if out:
                out.pop()
            out.extend(pts.tolist())
        want = len(out) if whole else 2
        need += want
        status = WHOLE if whole else LEG_FAILED
        if whole and cap_total is not None and used + want + 2 * (len(routes) - 1 - r) > cap_total:
            status = NO_ROOM
        if status != WHOLE:
            out = [wp[0].tolist(), wp[-1].tolist()]
        used += len(out)
        paths.append(np.array(out, dtype=np.float64).reshape(-1, 3)); rst.append(status)
    return dict(paths=paths, route_status=np.array(rst, np.int32), leg_status=np.array(lst, np.int32), levels=np.array(lev, np.int32),
                max_level_cells=np.array(mx, np.int32), need=need)


def box_map(rng, dim, frac, res=0.1, origin=(0.0, 0.0, 0.0)):
    """cells (int8, x fastest) of a map with random boxes of 100 until about `frac` of the cells are occupied"""
    nx, ny, nz = dim
    c = np.zeros((nz, ny, nx), np.int8)
    while c.mean() / 100.0 < frac:
        sx, sy, sz = rng.integers(1, 4), rng.integers(1, 5), rng.integers(1, nz + 1)
        x, y, z = rng.integers(0, nx - sx + 1), rng.integers(0, ny - sy + 1), rng.integers(0, nz - sz + 1)
        c[z:z + sz, y:y + sy, x:x + sx] = 100
    return c.reshape(-1)


def free_cell(rng, cells, dim):
    while True:
        c = [int(rng.integers(0, d)) for d in dim]
        if cells[c[0] + dim[0] * c[1] + dim[0] * dim[1] * c[2]] == 0:
            return c


def centre(c, origin, res, jitter=(0.0, 0.0, 0.0)):
    return [(c[i] + 0.5) * res + origin[i] + jitter[i] for i in range(3)]


def mixed_batch(dim, origin, res, seed=5, frac=0.04):
    """(cells, routes): a box map with some unknown cells and one free cell walled in on all six sides.  Routes 0, 1, 3, 4 have 0, 3, 0 and 3 gates at random
    free cells (off the centres); route 2 has its only gate inside a box (legs: goal not free, start not free); route 5 starts in an unknown cell, route 6 ends
    in one (the search crosses unknown cells, but an end must be free); route 7 ends in the walled-in cell (no path)."""
    rng = np.random.default_rng(seed)
    cells = box_map(rng, dim, frac)
    every = (np.arange(cells.size) % 97) == 0
    cells[every] = np.where(cells[every] == 0, -1, 100)                                            # some unknown cells
    pocket = [dim[0] // 2, dim[1] // 2, dim[2] // 2]
    grid = cells.reshape(dim[2], dim[1], dim[0])
    for st in STEPS:
        grid[pocket[2] + st[2], pocket[1] + st[1], pocket[0] + st[0]] = 100
    grid[pocket[2], pocket[1], pocket[0]] = 0
    occ = np.flatnonzero(cells == 100)
    box = int(occ[len(occ) // 2])
    unknown = [int(u) for u in np.flatnonzero(cells == -1)[[3, 11]]]
    cell_of = lambda i: [i % dim[0], i // dim[0] % dim[1], i // (dim[0] * dim[1])]                  # noqa: E731

    def free():
        while True:
            c = free_cell(rng, cells, dim)
            if c != pocket:
                return c
    routes = [np.array([centre(free(), origin, res, rng.uniform(-0.04, 0.04, 3)) for _ in range(g + 2)]) for g in (0, 3, 0, 3)]
    routes.insert(2, np.array([centre(free(), origin, res), centre(cell_of(box), origin, res), centre(free(), origin, res)]))
    routes.append(np.array([centre(cell_of(unknown[0]), origin, res), centre(free(), origin, res)]))
    routes.append(np.array([centre(free(), origin, res), centre(cell_of(unknown[1]), origin, res)]))
    routes.append(np.array([centre(free(), origin, res), centre(pocket, origin, res)]))
    return cells, routes


MIXED_ROUTE_STATUS = [0, 0, 1, 0, 0, 1, 1, 1]                                                      # of mixed_batch at roomy capacities
MIXED_LEG_FAILURES = {5: GOAL, 6: START, 12: START, 13: GOAL, 14: NO_PATH}                        # leg index -> status of the legs that fail


def simplified_path(m: Map, start, goal):
    """The vertices (points) of a leg after removeCornerPts forwards and backwards and removeLinePts, and the leg's sample points, from the level search."""
    st, cells, _, _ = level_search(m.cells, m.dim, m.float_to_int(start), m.float_to_int(goal))
    assert st == OK
    raw = [m.int_to_float(c) for c in cells]
    q = remove_corner_pts(m, raw)
    q = remove_line_pts(remove_corner_pts(m, q[::-1])[::-1])
    return q, np.array(sample_path(m, q), dtype=np.float64).reshape(-1, 3)


def walk_samples(m: Map, a, b):
    """max_diff of the sight-line walk from a to b (Map.ray_trace): the walk takes max_diff - 1 samples"""
    return int(max(abs((b[i] - a[i]) / m.res) for i in range(3)) / 0.8)


def edge_samples(p1, p2):
    """The samples samplePath takes on the edge p1 -> p2: its d accumulates 0.02 (it is not i * 0.02) for as long as d <= |p2 - p1|."""
    l = math.sqrt((p2[0] - p1[0]) ** 2 + (p2[1] - p1[1]) ** 2 + (p2[2] - p1[2]) ** 2)
    d, n = 0.0, 0
    while d <= l:
        n += 1
        d += 0.02
    return n


def walk_first_hit(m: Map, a, b, val=100):
    """(max_diff, the number n of the first sample of the sight-line walk a -> b on a cell >= val, or None): Map.ray_trace sample for sample, stopped at the
    first sample outside the map.  The walk's de-duplication of repeated cells cannot change the first hit."""
    diff = [b[i] - a[i] for i in range(3)]
    max_diff = int(max(abs(d / m.res) for d in diff) / 0.8)
    if max_diff == 0:
        return 0, None
    s = 1.0 / max_diff
    step = [d * s for d in diff]
    for n in range(1, max_diff):
        c = m.float_to_int([a[i] + step[i] * n for i in range(3)])
        if m.outside(c):
            break
        if m.cells[m.index(c)] >= val:
            return max_diff, n
    return max_diff, None


def corner_pass_logged(m: Map, path, log):
    """remove_corner_pts of the oracle, statement for statement, appending (a, b, max_diff, first blocked sample or None) to `log` for every chord it walks"""
    def cost(a, b):
        md, hit = walk_first_hit(m, a, b)
        log.append((a, b, md, hit))
        return math.inf if hit is not None else math.sqrt((a[0] - b[0]) ** 2 + (a[1] - b[1]) ** 2 + (a[2] - b[2]) ** 2)
    if len(path) < 2:
        return list(path)
    out = [path[0]]; prev = path[0]
    cost1 = cost(path[0], path[1])
    for i in range(1, len(path) - 1):
        p1, p2 = path[i], path[i + 1]
        cost2 = cost(p1, p2)
        cost3 = cost(prev, p2)
        if cost3 < cost1 + cost2:
            cost1 = cost3
        else:
            out.append(p1); cost1 = math.sqrt((p1[0] - p2[0]) ** 2 + (p1[1] - p2[1]) ** 2 + (p1[2] - p2[2]) ** 2); prev = p1
    out.append(path[-1])
    return out


def leg_log(m: Map, start, goal):
    """dict(raw, path, samples, chords) of one leg that the search finds: the raw cell centres, the vertices after the three passes, the sample points and
    the chords both corner passes walked.  The logged passes are held to the oracle's own (remove_corner_pts) here, vertex for vertex."""
    st, cells, _, _ = level_search(m.cells, m.dim, m.float_to_int(start), m.float_to_int(goal))
    assert st == OK, st
    raw = [m.int_to_float(c) for c in cells]
    chords = []
    q = corner_pass_logged(m, raw, chords)
    assert q == remove_corner_pts(m, raw)
    back = corner_pass_logged(m, q[::-1], chords)
    assert back == remove_corner_pts(m, q[::-1])
    path = remove_line_pts(back[::-1])
    return dict(raw=raw, path=path, samples=np.array(sample_path(m, path), dtype=np.float64).reshape(-1, 3), chords=chords)


def same_bits(a, b):
    a = np.ascontiguousarray(a, dtype=np.float64); b = np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))
