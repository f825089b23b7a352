"""numpy restatement of frx_trajectory_map_distance and frx_map_distance_fold (include/frx.h) - test infrastructure, not a test module.

Per fine piece the samples s_j = j (T / M), the position in the operation order of poly_eval<0> (frx_math.hpp), the cell by round((p - origin) / res - 0.5)
with C's rounding (halves away from zero), one look-up of the field.  The field value has no rounding of its own, so a row is exact wherever the cell is;
a piece is DECISION-SAFE when no sample lies within 1e-9 of a cell border, in cell units, on any axis - there the last bits of a position cannot move a sample
into the neighbouring cell.  Samples that are not numbers are outside the map and safe.
"""
import numpy as np

SAFE = 1e-9
FLAG_BELOW, FLAG_OUTSIDE, FLAG_NONFINITE = 1, 2, 4


def c_round(t):
    return np.trunc(t + np.copysign(0.5, t))


def before(a, ja, b, jb):
    """(value, key) a before b: not a number first, then the smaller value, then the lower key"""
    na, nb = a != a, b != b
    if na or nb:
        return na and (not nb or ja < jb)
    return a < b or (a == b and ja < jb)


def pieces(T, Cf, M, origin, dim, res, field):
    """rows (P, 4) = (DIST, WORST_T, WORST_CELL, OUTSIDE) and safe (P,) bool"""
    T = np.asarray(T, dtype=np.float64).reshape(-1)
    C = np.asarray(Cf, dtype=np.float64).reshape(-1, 6, 3)
    origin = np.asarray(origin, dtype=np.float64); dim = np.asarray(dim, dtype=np.int64); res = np.float64(res)
    field = np.asarray(field, dtype=np.float64).reshape(-1)
    rows = np.zeros((len(T), 4)); safe = np.ones(len(T), bool)
    j = np.arange(M + 1)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(len(T)):
            step = T[k] / np.float64(M)
            s1 = step * j.astype(np.float64)
            s2 = s1 * s1; s3 = s2 * s1; s4 = s2 * s2
            c = C[k]
            p = c[0][None, :] + c[1][None, :] * s1[:, None] + c[2][None, :] * s2[:, None] + c[3][None, :] * s3[:, None] + c[4][None, :] * s4[:, None] \
                + c[5][None, :] * (s4 * s1)[:, None]
            u = (p - origin[None, :]) / res
            t = u - 0.5
            r = c_round(t)
            frac = np.abs(t - np.floor(t) - 0.5)                          # distance of u from a border, 0 on it
            near = np.isfinite(t) & (frac < SAFE)
            safe[k] = not near.any()
            inside = np.isfinite(r).all(axis=1) & (r >= 0).all(axis=1) & (r < dim[None, :]).all(axis=1)
            rows[k, 3] = float((~inside).sum())
            best = None
            for jj in np.flatnonzero(inside):
                cell = int(r[jj, 0]) + int(dim[0]) * (int(r[jj, 1]) + int(dim[1]) * int(r[jj, 2]))
                v = field[cell]
                if best is None or before(v, jj, best[0], best[1]):
                    best = (v, int(jj), cell)
            if best is None:
                rows[k, :3] = (np.inf, -1.0, -1.0)
            else:
                rows[k, :3] = (best[0], step * np.float64(best[1]), float(best[2]))
    return rows, safe


def fold(rows, T, off, margin):
    """candidate rows (B, 4) and flags (B,) uint32; a candidate without pieces keeps a row of zeros and no flag"""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 4); T = np.asarray(T, dtype=np.float64).reshape(-1)
    B = len(off) - 1
    cand = np.zeros((B, 4)); flags = np.zeros(B, np.uint32)
    for b in range(B):
        t0 = np.float64(0.0)
        for k, gp in enumerate(range(off[b], off[b + 1])):
            r = rows[gp]
            if k == 0 or before(r[0], 1, cand[b, 0], 0):                  # strictly before: an equal later piece does not replace
                cand[b, 0] = r[0]; cand[b, 2] = r[2]
                cand[b, 1] = t0 + r[1] if r[2] >= 0.0 else -1.0
            cand[b, 3] = r[3] if k == 0 else cand[b, 3] + r[3]
            t0 = t0 + T[gp]
        if off[b + 1] == off[b]:
            continue
        flags[b] = (FLAG_BELOW if cand[b, 0] < margin else 0) | (FLAG_OUTSIDE if cand[b, 3] > 0.0 else 0) | (0 if np.isfinite(cand[b]).all() else FLAG_NONFINITE)
    return cand, flags
