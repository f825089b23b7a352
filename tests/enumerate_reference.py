"""Plain numpy restatement of enumerate() of fast-racing_amd/csrc/frx_geometry.cpp (the H -> V enumeration behind frx_enumerate_vertices and, on the device,
k_enumerate of frx_enumerate_kernel.hpp) - test infrastructure, not a test module.

Every expression is written out as explicit products and sums in the host's order, left to right (no dot, no einsum: numpy's elementwise multiply, add, subtract,
divide and sqrt are the correctly rounded IEEE operations, none fused), and the grid key is np.rint (round half to even, as nearbyint in the default mode).  Beside
the vertices and the verdict it returns what the host never shows: the RANK of every feasible triple in the lexicographic order of a < b < c, and each such rank's
key - from which the states of tests/enumerate_states.py assert where their duplicates and window edges lie.
"""
import itertools

import numpy as np

POLY_OK, POLY_UNBOUNDED, POLY_FLAT = 0, 1, 2
TOL, QUANT = 1e-9, 1e-7


def planes(rec):
    """rec [K][6] (outer normal, point) -> [K][4] (unit normal, offset)"""
    r = np.asarray(rec, dtype=np.float64).reshape(-1, 6)
    r0, r1, r2, r3, r4, r5 = (r[:, i] for i in range(6))
    with np.errstate(all="ignore"):
        nn = np.sqrt(r0 * r0 + r1 * r1 + r2 * r2)
        return np.stack([r0 / nn, r1 / nn, r2 / nn, (r0 * r3 + r1 * r4 + r2 * r5) / nn], axis=1)


def rank_of(K, a, b, c):
    """rank of the triple a < b < c among all triples of K indices in lexicographic order (exact integers)"""
    c3 = lambda n: n * (n - 1) * (n - 2) // 6
    m = K - a - 1
    i = b - a - 1
    return c3(K) - c3(K - a) + i * (2 * m - i - 1) // 2 + (c - b - 1)


def triples(K):
    return np.array(list(itertools.combinations(range(K), 3)), dtype=np.int64).reshape(-1, 3)


def solve(pl, T):
    """the points of the plane triples T [n][3] and which of them the determinant keeps: (keep, x0, x1, x2)"""
    A, B, C = pl[T[:, 0]], pl[T[:, 1]], pl[T[:, 2]]
    with np.errstate(all="ignore"):
        cx = B[:, 1] * C[:, 2] - B[:, 2] * C[:, 1]; cy = B[:, 2] * C[:, 0] - B[:, 0] * C[:, 2]; cz = B[:, 0] * C[:, 1] - B[:, 1] * C[:, 0]
        det = A[:, 0] * cx + A[:, 1] * cy + A[:, 2] * cz
        keep = ~(np.abs(det) <= 1e-10)
        ax = C[:, 1] * A[:, 2] - C[:, 2] * A[:, 1]; ay = C[:, 2] * A[:, 0] - C[:, 0] * A[:, 2]; az = C[:, 0] * A[:, 1] - C[:, 1] * A[:, 0]
        bx = A[:, 1] * B[:, 2] - A[:, 2] * B[:, 1]; by = A[:, 2] * B[:, 0] - A[:, 0] * B[:, 2]; bz = A[:, 0] * B[:, 1] - A[:, 1] * B[:, 0]
        x0 = (A[:, 3] * cx + B[:, 3] * ax + C[:, 3] * bx) / det
        x1 = (A[:, 3] * cy + B[:, 3] * ay + C[:, 3] * by) / det
        x2 = (A[:, 3] * cz + B[:, 3] * az + C[:, 3] * bz) / det
    return keep, x0, x1, x2


def triple_point(rec, a, b, c):
    """the point of planes a < b < c of rec as the enumeration computes it (its feasibility is not judged)"""
    _, x0, x1, x2 = solve(planes(rec), np.array([[a, b, c]], dtype=np.int64))
    return np.array([x0[0], x1[0], x2[0]])


def enumerate_ref(rec):
    """dict(vertices [nv][3] in the host's order, verdict, ranks [F] of the feasible triples ascending, keys [F][3] int64, points [F][3], owner [nv] = the rank
    whose point each vertex is, spans = some plane is not parallel to some pair's line, ray_pairs = the ranks of the plane pairs with a free ray,
    slacks [K] = every plane's slack at the centroid, or None where the host does not get that far)"""
    pl = planes(rec)
    K = len(pl)
    T = triples(K)
    feas, x0, x1, x2 = solve(pl, T)
    with np.errstate(all="ignore"):
        for k in range(K):
            feas &= pl[k, 0] * x0 + pl[k, 1] * x1 + pl[k, 2] * x2 <= pl[k, 3] + TOL
    ranks = np.nonzero(feas)[0]
    pts = np.stack([x0[ranks], x1[ranks], x2[ranks]], axis=1)
    keys = np.rint(pts / QUANT).astype(np.int64)
    first = {}
    for i, key in enumerate(map(tuple, keys)):                              # first occurrence wins
        first.setdefault(key, i)
    order = sorted(first)                                                   # lexicographic over three signed integers
    owner = np.array([ranks[first[key]] for key in order], dtype=np.int64)
    verts = np.array([pts[first[key]] for key in order], dtype=np.float64).reshape(-1, 3)

    # verdict
    P = np.array(list(itertools.combinations(range(K), 2)), dtype=np.int64).reshape(-1, 2)
    A, B = pl[P[:, 0]], pl[P[:, 1]]
    with np.errstate(all="ignore"):
        u0 = A[:, 1] * B[:, 2] - A[:, 2] * B[:, 1]; u1 = A[:, 2] * B[:, 0] - A[:, 0] * B[:, 2]; u2 = A[:, 0] * B[:, 1] - A[:, 1] * B[:, 0]
        un = np.sqrt(u0 * u0 + u1 * u1 + u2 * u2)
        live = ~(un <= 1e-10)
        u0 = u0 / un; u1 = u1 / un; u2 = u2 / un
        sp = np.zeros(len(P), bool); fneg = np.ones(len(P), bool); fpos = np.ones(len(P), bool)
        for k in range(K):
            dot = pl[k, 0] * u0 + pl[k, 1] * u1 + pl[k, 2] * u2
            sp |= np.abs(dot) > 1e-10
            fneg &= -dot <= 1e-12
            fpos &= dot <= 1e-12
    spans = bool((live & sp).any()); ray = bool((live & (fneg | fpos)).any())
    ray_pairs = np.nonzero(live & (fneg | fpos))[0]                          # ranks of the plane pairs a < b, in lexicographic order, that have a free ray
    slacks = None
    verdict = POLY_OK
    if not spans or ray:
        verdict = POLY_UNBOUNDED
    elif len(verts) < 4:
        verdict = POLY_FLAT
    else:
        c = [0.0, 0.0, 0.0]
        for v in verts:                                                     # in vertex order, one addition at a time
            c[0] += float(v[0]); c[1] += float(v[1]); c[2] += float(v[2])
        c = [q / float(len(verts)) for q in c]
        slack = np.finfo(np.float64).max
        slacks = np.empty(K)
        for k in range(K):
            s = float(pl[k, 3]) - (float(pl[k, 0]) * c[0] + float(pl[k, 1]) * c[1] + float(pl[k, 2]) * c[2])
            slacks[k] = s
            slack = s if s < slack else slack                               # std::min
        if not slack > TOL:
            verdict = POLY_FLAT
    return dict(vertices=verts, verdict=verdict, ranks=ranks, keys=keys, points=pts, owner=owner, spans=spans, ray_pairs=ray_pairs, slacks=slacks)


def host_enum(frx, rec):
    """frx_enumerate_vertices on rec [K][6]: (nv, vertices [nv][3] or None when the host refuses the polytope, verdict)"""
    rec = np.ascontiguousarray(rec, dtype=np.float64).reshape(-1)
    if len(rec) // 6 >= 128:                                                # the large states take the host seconds: once a process, the result read-only
        key = rec.tobytes()
        if key not in _large:
            _large[key] = _host_enum(frx, rec)
            if _large[key][1] is not None:
                _large[key][1].setflags(write=False)
        return _large[key]
    return _host_enum(frx, rec)


_large = {}


def _host_enum(frx, rec):
    import ctypes as C
    K = len(rec) // 6
    nv = C.c_int()
    rc = frx.lib().frx_enumerate_vertices(K, rec, None, 0, C.byref(nv))
    if rc == -4:                                                            # FRX_ERR_EMPTY_POLYTOPE: the text names the verdict
        return nv.value, None, POLY_UNBOUNDED if b"unbounded" in frx.lib().frx_last_error() else POLY_FLAT
    assert rc == 0, (rc, frx.lib().frx_last_error())
    out = np.zeros(3 * max(nv.value, 1))
    assert frx.lib().frx_enumerate_vertices(K, rec, out.ctypes.data, nv.value, C.byref(nv)) == 0
    return nv.value, out[:3 * nv.value].reshape(-1, 3), POLY_OK
