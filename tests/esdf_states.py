"""Crafted maps for the voxel map's distance field (frx_map_esdf, frx_esdf_kernel.hpp) - test infrastructure, not a test module.

Dimensions: the degenerate grids, odd sizes, and one grid on each side of every boundary the kernels have - a workgroup is 256 lanes (THREADS), over the flat
(x, y) columns in the z pass, over x in the column-distance pass, over the flat cells in the y pass, and a stride along x in the x pass: 255 / 256 / 257 columns, cells and cells along x.
Contents: every kind of site set, the empty ones included.  LIMIT is the accepted line limit along x; one cell more is FRX_ERR_CAPACITY.
"""
import numpy as np

THREADS = 256
LIMIT = 8192                                                             # ESDF_MAX_LINE (fast-racing_amd/csrc/frx_esdf_plan.hpp)
MAX_DIM = 16384                                                          # ESDF_MAX_DIM

DIMS = [(1, 1, 1), (2, 1, 1), (5, 1, 3), (1, 65, 1), (64, 3, 2), (65, 64, 3), (257, 2, 2),
        (255, 1, 1), (256, 1, 1), (16, 16, 1), (64, 4, 1), (3, 85, 2), (1, 1, 257)]
RES = (0.1, 0.25, 0.3)                                                   # 0.1 and 0.3 are not dyadic: res * sqrt(v) rounds


def contents(dim, rng):
    """(name, cells int8 flat, x fastest) for every kind of content"""
    nx, ny, nz = dim
    n = nx * ny * nz
    free = np.zeros(n, np.int8)
    out = [("no occupied cell", free.copy()), ("all occupied", np.full(n, 100, np.int8)), ("all unknown", np.full(n, -1, np.int8))]
    c = free.copy(); c[n - 1] = 100
    out.append(("one site in a corner", c))
    c = np.full(n, 100, np.int8); c[n // 3] = 0
    out.append(("one free cell in a full map", c))
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    out.append(("checkerboard", np.where((x + y + z) % 2 == 0, 100, 0).astype(np.int8).ravel()))
    out.append(("a full plane of sites", np.where(x == nx // 2, 100, 0).astype(np.int8).ravel()))
    out.append(("a full plane of unknown cells in an occupied map", np.where(y == ny // 2, -1, 100).astype(np.int8).ravel()))
    for frac in (0.01, 0.3):
        out.append((f"random {frac}", np.where(rng.random(n) < frac, 100, 0).astype(np.int8)))
    out.append(("values", rng.choice(np.array([-1, 0, 1, 99, 100], np.int8), n)))
    out.append(("unknown with one site and one free cell", _two(n)))
    return out


def _two(n):
    c = np.full(n, -1, np.int8)
    c[0] = 1
    c[n - 1] = 0
    return c


def states():
    """(label, dim, res, cells) over every dimension and content, plus the map at the line limit"""
    rng = np.random.default_rng(20)
    out = []
    for k, dim in enumerate(DIMS):
        for name, cells in contents(dim, rng):
            out.append((f"{dim} {name}", dim, RES[k % len(RES)], cells))
    c = np.zeros(LIMIT, np.int8); c[[5, LIMIT - 300]] = 100; c[[6, 4000]] = -1
    out.append((f"({LIMIT}, 1, 1) at the line limit", (LIMIT, 1, 1), 0.1, c))
    return out


_STATES = None


def all_states():
    global _STATES
    if _STATES is None:
        _STATES = states()
    return _STATES
