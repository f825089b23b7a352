"""Referee of the voxel map's distance field (frx_map_esdf, include/frx.h) - test infrastructure, not a test module.

numpy on int64.  Per axis a brute-force min-plus over the whole line, out[i] = min over q of g[q] + (i - q)^2: neither the host's lower envelope
(frx_esdf_host.hpp) nor the device's search outwards from the cell (frx_esdf_kernel.hpp).  brute_squared is the definition itself, the minimum over all
pairs (cell, site), for maps small enough to afford it; tests/test_esdf_cpu.py pins the one against the other.

Cells are stored x fastest: an array of shape (nz, ny, nx).  A cell > 0 is occupied, == 0 is free, -1 is neither (map_util.h:322-326).
"""
import numpy as np

INF = np.int64(1) << 40                                                  # above every finite value, 3 x 16383^2


def grid(cells, dim):
    return np.asarray(cells, dtype=np.int8).reshape(int(dim[2]), int(dim[1]), int(dim[0]))


def axis_pass(g, axis):
    """min-plus of g (int64, INF = no site) with the parabola along `axis`, in slabs of output cells so that a slab's (i, q) table stays small"""
    g = np.moveaxis(g, axis, -1)
    n = g.shape[-1]
    q = np.arange(n, dtype=np.int64)
    out = np.empty_like(g)
    lines = max(g.size // n, 1)
    slab = max(1, (1 << 22) // (n * lines))
    for i0 in range(0, n, slab):
        i = np.arange(i0, min(i0 + slab, n), dtype=np.int64)
        cost = g[..., None, :] + (i[:, None] - q[None, :]) ** 2           # (..., slab, n)
        out[..., i0:i0 + len(i)] = cost.min(axis=-1)
    out = np.where(out >= INF, INF, out)
    return np.moveaxis(out, -1, axis)


def squared(site):
    """site: bool (nz, ny, nx) -> int64 squared distance in cells to the nearest site, INF where there is none"""
    g = np.where(site, np.int64(0), INF)
    for axis in (0, 1, 2):                                               # z, y, x: the order does not matter to a minimum
        g = axis_pass(g, axis)
    return g


def brute_squared(site):
    """the definition: min over all sites of the squared distance, for small maps"""
    nz, ny, nx = site.shape
    zz, yy, xx = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    pts = np.stack([zz.ravel(), yy.ravel(), xx.ravel()], axis=1).astype(np.int64)
    s = pts[site.ravel()]
    if len(s) == 0:
        return np.full(site.shape, INF)
    d = ((pts[:, None, :] - s[None, :, :]) ** 2).sum(axis=2).min(axis=1)
    return d.reshape(site.shape)


def metres(d2, res):
    """res * sqrt(d2), one correctly rounded square root and one product; +inf without a site"""
    with np.errstate(invalid="ignore"):
        return np.where(d2 >= INF, np.inf, np.float64(res) * np.sqrt(d2.astype(np.float64)))


def fields(cells, dim, res, squared_of=squared):
    """dict(pos, neg, all) flat float64 over the cells, and d2_occ / d2_free (int64, INF = none)"""
    c = grid(cells, dim)
    occ, fre = squared_of(c > 0), squared_of(c == 0)
    pos, neg = metres(occ, res), metres(fre, res)
    with np.errstate(invalid="ignore"):
        both = np.where(neg > 0.0, pos + (-neg + np.float64(res)), pos)   # map_util.h:241-243, the parenthesis first
    both = np.where(np.isnan(both), np.float64(np.nan), both)           # inf - inf: the sign of that NaN is the machine's; the library writes the plain quiet NaN
    return dict(pos=pos.ravel(), neg=neg.ravel(), all=both.ravel(), d2_occ=occ.ravel(), d2_free=fre.ravel())


def same_bits(a, b):
    a = np.ascontiguousarray(a, dtype=np.float64); b = np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))
