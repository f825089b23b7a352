"""Scenes of the batched corridor generation (frx_corridor_generate_batch, frx_chain_kernel.hpp) - test infrastructure, not a test module.

  world()          nine ragged paths through ONE obstacle cloud and ONE voxel map marked from it: routes through 1-4 gates at 0.5 m spacing (50-135 points,
                   as _scene of test_next_rows.py builds them, the last leg 14.8 m), a 2-point path in free space and a path inside a block of occupied cells, 0.9 m spacing, whose
                   every step is blocked (the cells are marked from a wall of points that is NOT part of the cloud: the cells there are the local box alone).
  dense_path()     a straight free stretch at 0.01 m spacing: with the right max_seg / box length the first stop or the exit index falls on lane 255 of a
                   window of 256 path points, or on lane 0 or 1 of the next window.
  overflow worlds  one path beside a clump of 5000 cloud points (more than a cell's 4096-point buffer), far from its neighbours.
  sight_pairs()    hand-made rays on a random occupancy grid of 0.1 m cells: axis-aligned between cell centres 2, 4, 10 and 20 cells apart (the 10-cell ray's
                   third sample lies exactly on a cell border in exact arithmetic: (i + 3) res, where round(x / res - 0.5) is decided by the last bit - a
                   fused multiply-add in a + step * n flips it), rays that leave the map, rays that start or end in an occupied cell; plus random ones.

The device and the host differ in the last bits INSIDE a cell (trigonometry, contraction), so every scene handed out is decision-safe for the host chain
(decision_margins): over the host's cells and all path points | n.(P - p) - 1e-10 | >= 1e-6 (tangent and box planes), and over all point pairs of a path
| |P_i - P_k| - max_seg | >= 1e-6.  The seeds below were chosen on the CPU so that this holds; a seed that fails is replaced, not tolerated.
"""
import numpy as np

BBOX = np.array([4.0, 4.0, 2.5])
MAP_HEIGHT, MAX_SEG, SAFE = 3.0, 4.0, 1e-6
MAP_ORIGIN, MAP_DIM, MAP_RES = [-30.0, -6.0, -0.5], [240, 320, 18], 0.25      # x in [-30, 30], y in [-6, 74], z in [-0.5, 4]
WORLD_SEEDS = [(1, 4), (2, 3), (3, 2), (4, 1), (5, 4), (6, 3), (7, 2)]       # (seed, gates) of the seven routes
FOG_LO, FOG_HI = np.array([22.0, 0.0, 0.5]), np.array([28.0, 20.0, 2.5])      # the block of occupied cells


def route(sc, seed, n_gates):
    g = sc.SplitMix64(seed)
    gates = sc.make_gates(g, n_gates)
    wps = np.vstack([[0.0, 0.0, 1.0], gates, gates[-1] + [0.0, 14.8, 0.0]])                 # (15 m would put points exactly max_seg apart)
    path = [wps[0]]
    for a, b in zip(wps[:-1], wps[1:]):                                       # dense front-end-like path, 0.5 m spacing
        m = int(np.ceil(np.linalg.norm(b - a) / 0.5))
        path += [a + (b - a) * (t / m) for t in range(1, m + 1)]
    return np.array(path)


def cloud_around(rng, paths, n_obs, clear=0.6, spread=3.0):
    """n_obs points scattered around the paths' points, none closer than `clear` to any point of any path"""
    pts = np.vstack(paths); obs = []
    while len(obs) < n_obs:
        q = pts[rng.integers(len(pts))] + rng.normal(0, spread, 3)
        if 0.0 < q[2] < 3.0 and np.min(np.linalg.norm(pts - q, axis=1)) > clear:
            obs.append(q)
    return np.array(obs)


def voxel_map(frx, cloud, extra=None):
    vm = frx.VoxelMap(MAP_ORIGIN, MAP_DIM, MAP_RES)
    vm.mark_cloud(cloud)
    if extra is not None:
        vm.mark_cloud(extra)
    return vm


def fog_points():
    """one point in every cell of the block FOG_LO .. FOG_HI"""
    ax = [np.arange(FOG_LO[d] + MAP_RES / 2, FOG_HI[d], MAP_RES) for d in range(3)]
    return np.stack(np.meshgrid(*ax, indexing="ij"), axis=-1).reshape(-1, 3)


def decision_margins(frx, path, cloud, bbox, map_height, max_seg, vm):
    """(smallest | n.(P - p) - 1e-10 | over the host chain's tangent and box planes and all path points, smallest | |P_i - P_k| - max_seg | over all pairs)"""
    cells = frx.corridor_generate(path, cloud, bbox, map_height, max_seg=max_seg, blocked=vm)
    m_plane = np.inf
    for H in cells:
        H = H[:, :-2]                                                        # floor and ceiling are appended after the exit test
        sd = np.einsum("dk,ndk->nk", H[:3], path[:, :, None] - H[3:][None])
        m_plane = min(m_plane, np.abs(sd - 1e-10).min())
    d = np.linalg.norm(path[:, None, :] - path[None, :, :], axis=2)
    return m_plane, np.abs(d - max_seg).min()


def assert_safe(frx, paths, cloud, bbox, map_height, max_seg, vm):
    for b, p in enumerate(paths):
        mp, md = decision_margins(frx, p, cloud, bbox, map_height, max_seg, vm)
        assert mp >= SAFE and md >= SAFE, (b, mp, md)


_world = {}


def world(frx, sc):
    """dict(paths [9], cloud, vm, ref = host chain per path with the map, ref_free = without); built and self-checked once"""
    if not _world:
        rng = np.random.default_rng(2024)
        routes = [route(sc, s, g) for s, g in WORLD_SEEDS]
        two = np.array([[25.0, 30.0, 1.0], [25.0, 31.0, 1.0]])
        fogged = np.array([[25.0, 1.0 + 0.9 * t, 1.5] for t in range(19)])
        paths = [routes[0], two, routes[1], routes[2], fogged] + routes[3:]
        assert len(paths) == 9 and all(30 <= len(r) <= 150 for r in routes)
        cloud = cloud_around(rng, routes, 3000)
        assert np.linalg.norm(cloud - two[0], axis=1).min() > 8.0 and np.linalg.norm(cloud[:, None, :] - fogged[None], axis=2).min() > 8.0
        vm = voxel_map(frx, cloud, fog_points())
        assert all(vm.is_blocked(a, b) for a, b in zip(fogged[:-1], fogged[1:]))
        assert_safe(frx, paths, cloud, BBOX, MAP_HEIGHT, MAX_SEG, vm)
        assert_safe(frx, paths, cloud, BBOX, MAP_HEIGHT, MAX_SEG, None)
        _world.update(paths=paths, cloud=cloud, vm=vm,
                      ref=[frx.corridor_generate(p, cloud, BBOX, MAP_HEIGHT, MAX_SEG, blocked=vm) for p in paths],
                      ref_free=[frx.corridor_generate(p, cloud, BBOX, MAP_HEIGHT, MAX_SEG) for p in paths])
    return _world


def small_scene(frx, sc, seed, n_gates, n_obs):
    """one route in a cloud of its own (400-3000 points) with its map"""
    rng = np.random.default_rng(seed)
    path = route(sc, seed, n_gates)
    cloud = cloud_around(rng, [path], n_obs)
    vm = voxel_map(frx, cloud)
    assert_safe(frx, [path], cloud, BBOX, MAP_HEIGHT, MAX_SEG, vm)
    return path, cloud, vm


# ---- window edges -----------------------------------------------------------------------------------------------------------------------------------
DENSE_N, DENSE_STEP = 800, 0.01
# (max_seg, box length): the first stop of step 0 is point 256 / 257 / 258 = lane 255 of the first window of 256 points (which starts at point 1), lane 0
# and lane 1 of the second; and with max_seg 1.005 (k = 100) the first point outside the box is k + 255 / 256 / 257
EDGE_CASES = [(2.555, 4.005), (2.565, 4.005), (2.575, 4.005), (1.005, 2.545), (1.005, 2.555), (1.005, 2.565)]


def dense_path():
    return np.array([[-20.0, 2.0 + DENSE_STEP * t, 1.25] for t in range(DENSE_N)])


def dense_scene(frx):
    rng = np.random.default_rng(31)
    path = dense_path()
    cloud = cloud_around(rng, [path[::10]], 400, clear=4.3, spread=5.0)          # a free stretch: no cloud point inside a cell's local box along it
    for ms, bx in EDGE_CASES:
        assert_safe(frx, [path], cloud, np.array([bx, 4.0, 2.5]), MAP_HEIGHT, ms, None)
    # the edges are where the docstring says: recompute step 0's stop and exit with exact integers
    for ms, bx in EDGE_CASES[:3]:
        assert int(np.argmax(np.arange(DENSE_N) * DENSE_STEP >= ms)) in (256, 257, 258)
    return path, cloud


# ---- overflows --------------------------------------------------------------------------------------------------------------------------------------
def clump_world(frx, sc):
    """the world's cloud plus 5000 points in a ball of radius 0.3, 1.5 m beside a straight path at x = -28 that no other path comes near"""
    w = world(frx, sc)
    rng = np.random.default_rng(99)
    lone = np.array([[-28.0, 10.0 + 0.45 * t, 1.5] for t in range(23)])
    v = rng.normal(0, 1, (5000, 3)); v *= (0.3 * rng.uniform(0, 1, (5000, 1)) ** (1 / 3)) / np.linalg.norm(v, axis=1, keepdims=True)
    clump = np.array([-26.5, 15.0, 1.5]) + v
    assert np.linalg.norm(np.vstack(w["paths"])[:, :2] - np.array([-26.5, 15.0]), axis=1).min() > 6.5 + 0.3          # outside every other path's local boxes
    return lone, np.vstack([w["cloud"], clump])


# ---- sight lines ------------------------------------------------------------------------------------------------------------------------------------
SIGHT_ORIGIN, SIGHT_DIM, SIGHT_RES = [-1.3, 0.7, 0.0], [40, 40, 40], 0.1


def sight_map(frx):
    rng = np.random.default_rng(5)
    cells = np.where(rng.uniform(size=40 * 40 * 40) < 0.12, 100, 0).astype(np.int8)
    return frx.VoxelMap(SIGHT_ORIGIN, SIGHT_DIM, SIGHT_RES, cells)


def centre(c):
    return (np.asarray(c, dtype=np.float64) + 0.5) * SIGHT_RES + np.array(SIGHT_ORIGIN)     # intToFloat, map_util.h:389-392


def sight_pairs(vm):
    """dict(name -> (a [n][3], b [n][3])) of hand-made rays, and 'random'"""
    rng = np.random.default_rng(6)
    occ = vm.cells.reshape(SIGHT_DIM[::-1])                                  # [z][y][x]
    out = {}
    for span in (2, 4, 10, 20):
        a, b = [], []
        for axis in range(3):
            for sign in (1, -1):
                for _ in range(40):
                    c0 = rng.integers(0, 40, 3)
                    c0[axis] = rng.integers(0, 40 - span) if sign > 0 else rng.integers(span, 40)
                    c1 = c0.copy(); c1[axis] += sign * span
                    a.append(centre(c0)); b.append(centre(c1))
        out[f"span{span}"] = (np.array(a), np.array(b))
    a, b = [], []
    for axis in range(3):                                                   # rays that leave the map: the far end 5 to 30 cells outside
        for sign in (1, -1):
            for _ in range(20):
                c0 = rng.integers(0, 40, 3); c1 = c0.copy()
                c1[axis] = 40 + rng.integers(5, 30) if sign > 0 else -rng.integers(5, 30)
                a.append(centre(c0)); b.append(centre(c1) + rng.uniform(-0.04, 0.04, 3))
    out["leaving"] = (np.array(a), np.array(b))
    full = np.argwhere(occ == 100)[:, ::-1]
    a, b = [], []
    for k in range(60):                                                     # one end inside an occupied cell (the end cells themselves are not sampled)
        c0 = full[rng.integers(len(full))]; q = centre(c0) + rng.uniform(-0.04, 0.04, 3)
        r = q + rng.normal(0, 1, 3) * np.array([0.6, 0.6, 0.6])
        (a if k % 2 else b).append(q); (b if k % 2 else a).append(r)
    out["occupied_end"] = (np.array(a), np.array(b))
    lo, hi = np.array(SIGHT_ORIGIN), np.array(SIGHT_ORIGIN) + SIGHT_RES * 40
    a = rng.uniform(lo - 0.3, hi + 0.3, (400, 3)); b = a + rng.normal(0, 1, (400, 3)) * rng.uniform(0.05, 1.5, (400, 1))
    out["random"] = (a, b)
    return out


def border_samples(a, b):
    """distance of every sample coordinate's x / res - 0.5 to the nearest half-integer (where round() flips), smallest over the walk of ray a-b, in float64
    as the host forms it"""
    d = b - a
    md = int(np.max(np.abs(d / SIGHT_RES)) / 0.8)
    s = 1.0 / md
    best = np.inf
    for n in range(1, md):
        q = ((a + (d * s) * n) - np.array(SIGHT_ORIGIN)) / SIGHT_RES - 0.5
        best = min(best, np.abs(q - np.floor(q) - 0.5).min())
    return best
