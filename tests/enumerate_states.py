"""States of the batched vertex enumeration (frx_enumerate_vertices_batch, k_enumerate of frx_enumerate_kernel.hpp) - test infrastructure, not a test module.
Every state is a record array [K][6] (outer normal, point), the input of frx_enumerate_vertices.

  tetrahedron()       K = 4: the smallest polytope, C(4, 3) = 4 triples, all four feasible.
  cube()              K = 6, centred on the origin: negative grid keys, and ties in the first (and second) key component that the sort must break by the next.
  pyramid(d)          d side planes through ONE apex over a base plane, turned by a generic rotation and shifted.  All C(d, 3) triples of side planes meet
                      in the apex, each with its own last bits: at d = 40 that is 9 880 feasible triples of one grid key, spread over 42 windows of 256
                      ranks; all but the first must be dropped and the surviving coordinates are the first's.
  sphere(K, seed)     random planes around a sphere, each tangent to a sphere of its own radius in [1, 1.35]: some planes are redundant, the rest meet three at
                      a time (one feasible triple per vertex).  sphere(62, SEED_62) has exactly 82 vertices (the capacity edge).
  relabel(rec, r)     the same polytope with its planes renumbered so that the triple of one vertex has rank r: r = 255, 256, 257 puts it on the last lane of
                      the kernel's first window of 256 ranks and on lanes 0 and 1 of the second (K = 13: C(13, 3) = 286 = one window plus 30); r = 63, 64, 65
                      on the edge between the staging areas of the kernel's first two waves; K = 12 has 220 triples, a part-filled single window, with the
                      vertex on its last rank 219.
  open_cube()         the cube without one face: unbounded.       two_cubes()   two unit cubes sharing a face as ONE 12-plane task: flat, 4 vertices.

Above 64 planes and 256 vertices (the kernel's workgroup is four waves of 64 lanes, one lane per plane; its order loop takes 256 vertices a trip):
  sphere(K, 1)        K in CEILING_K = 63 ... 256: the plane count on either side of every wave edge and at the ceiling of 256.
  sphere(256, s, 0.0) every plane tangent to ONE sphere: none is redundant, 2 K - 4 = 508 vertices, one feasible triple each.
  prism(d)            d side planes tangent to a cylinder and two caps, turned and shifted like the pyramid: 2 d vertices from K = d + 2 planes; for even d the
                      opposite sides are antiparallel, so triples and pairs of them are skipped for their determinant and their cross product.
  pyramid(254 | 255)  255 and 256 vertices from 255 and 256 planes; C(255, 3) = 2 731 135 feasible triples of one key over 10 669 windows.
  flat_late()         64 redundant planes far outside, then two_cubes(): flat, and only planes of index >= 64 have no slack at the centroid.
  open_late()         64 redundant planes far outside with n_z > 0, then open_cube() (open towards -z): unbounded, and the first plane pair with a free ray comes
                      after every pair of the far planes.
  open_sides()        the 70 sides of prism(70) without the caps: the normals do not span, unbounded, no vertex.
"""
import numpy as np

SEED_13, SEED_12, SEED_62 = 5, 0, 9
CEILING_K = (63, 64, 65, 128, 129, 192, 193, 255, 256)
CEILING_NV = (68, 76, 76, 106, 106, 136, 122, 140, 142)                      # vertices of sphere(K, 1), K in CEILING_K
FAR_RADIUS, FAR_PLANES, FAR_SEED = 30.0, 64, 7
ROT_AXIS, ROT_ANGLE, SHIFT = np.array([0.3, -0.5, 0.8]), 0.7, np.array([1.234567, -2.345678, 0.876543])


def records(normals, points):
    return np.ascontiguousarray(np.concatenate([np.asarray(normals, dtype=np.float64), np.asarray(points, dtype=np.float64)], axis=1))


def tetrahedron():
    n = np.array([[-1.0, 0, 0], [0, -1.0, 0], [0, 0, -1.0], [1.0, 1.0, 1.0]])
    p = np.array([[0.0, 0, 0], [0, 0, 0], [0, 0, 0], [1.0, 0, 0]])
    return records(n, p)


def cube(half=1.0, centre=(0.0, 0.0, 0.0)):
    n = np.array([[1.0, 0, 0], [-1.0, 0, 0], [0, 1.0, 0], [0, -1.0, 0], [0, 0, 1.0], [0, 0, -1.0]])
    return records(n, np.asarray(centre) + half * n)


def open_cube():
    return cube()[:5]


def two_cubes():
    return np.concatenate([cube(0.5, (0.5, 0.5, 0.5)), cube(0.5, (1.5, 0.5, 0.5))])


def rotation(axis, angle):
    k = np.asarray(axis, dtype=np.float64); k = k / np.linalg.norm(k)
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * (Kx @ Kx)


def pyramid(d, height=1.5, slope=0.8):
    th = 2 * np.pi * (np.arange(d) + 0.25) / d
    n = np.stack([np.cos(th), np.sin(th), np.full(d, slope)], axis=1)       # side planes through the apex (0, 0, height)
    n = np.concatenate([n, [[0.0, 0.0, -1.0]]])                             # the base z >= 0, last
    p = np.concatenate([np.tile([0.0, 0.0, height], (d, 1)), [[0.0, 0.0, 0.0]]])
    R = rotation(ROT_AXIS, ROT_ANGLE)
    return records(n @ R.T, p @ R.T + SHIFT)


def prism(d, half=0.5):
    th = 2 * np.pi * (np.arange(d) + 0.25) / d
    side = np.stack([np.cos(th), np.sin(th), np.zeros(d)], axis=1)          # tangent to the unit cylinder around z
    n = np.concatenate([side, [[0.0, 0.0, 1.0], [0.0, 0.0, -1.0]]])         # the caps z = +-half, last
    p = np.concatenate([side, [[0.0, 0.0, half], [0.0, 0.0, -half]]])
    R = rotation(ROT_AXIS, ROT_ANGLE)
    return records(n @ R.T, p @ R.T + SHIFT)


def open_sides():
    return prism(70)[:70]


def far_planes(upward=False):
    """FAR_PLANES planes tangent to the sphere of radius FAR_RADIUS around the origin: redundant beside the cubes; upward: every normal has n_z > 0 and a
    horizontal part"""
    rng = np.random.default_rng(FAR_SEED)
    n = rng.normal(0, 1, (FAR_PLANES, 3)); n /= np.linalg.norm(n, axis=1, keepdims=True)
    if upward:
        n[:, 2] = np.abs(n[:, 2])
    return records(n, FAR_RADIUS * n)


def flat_late():
    return np.concatenate([far_planes(), two_cubes()])


def open_late():
    return np.concatenate([far_planes(upward=True), open_cube()])


def sphere(K, seed, spread=0.35):
    rng = np.random.default_rng(seed)
    n = rng.normal(0, 1, (K, 3)); n /= np.linalg.norm(n, axis=1, keepdims=True)
    rad = 1.0 + spread * rng.uniform(0, 1, (K, 1))
    centre = np.array([0.4, -1.1, 2.2])
    return records(n, centre + rad * n)


def unrank(K, r):
    """the triple of rank r in lexicographic order (exact integers, by counting)"""
    for a in range(K - 2):
        n = (K - a - 1) * (K - a - 2) // 2
        if r < n:
            for b in range(a + 1, K - 1):
                if r < K - b - 1:
                    return a, b, b + 1 + r
                r -= K - b - 1
        r -= n
    raise ValueError(r)


def relabel(rec, triple, r):
    """rec with its planes renumbered so that the planes `triple` stand at the indices of the triple of rank r (the others keep their relative order)"""
    K = len(rec)
    target = unrank(K, r)
    rest = [k for k in range(K) if k not in triple]
    out = np.empty_like(rec); it = iter(rest)
    for k in range(K):
        out[k] = rec[triple[target.index(k)]] if k in target else rec[next(it)]
    return out


WINDOW_RANKS_13 = (255, 256, 257, 63, 64, 65)
WINDOW_RANKS_12 = (219, 0)


def window_states(ref):
    """list of (name, rec, rank, key): the K = 13 and K = 12 sphere polytopes relabelled so that the feasible triple of their first vertex has that rank;
    `ref` = enumerate_reference.enumerate_ref"""
    import enumerate_reference as er
    out = []
    for K, seed, ranks in ((13, SEED_13, WINDOW_RANKS_13), (12, SEED_12, WINDOW_RANKS_12)):
        rec = sphere(K, seed)
        e = ref(rec)
        T = er.triples(K)
        triple = tuple(int(v) for v in T[e["owner"][0]])
        key = tuple(int(v) for v in e["keys"][list(e["ranks"]).index(e["owner"][0])])
        for r in ranks:
            out.append((f"K{K}_rank{r}", relabel(rec, triple, r), r, key))
    return out
