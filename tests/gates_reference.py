"""Restatement of the exact gate passage certificate (frx_trajectory_gates, include/frx.h) - test infrastructure, not a test module.

Two independent things live here.

1. `gate_row` / `rows` / `flags_of`: the kernel's arithmetic restated operation by operation in float64 (Python floats: every + - * / is one correctly
   rounded IEEE operation, nothing is fused; math.sqrt is correctly rounded).  It is the referee for bit identity.  The roots come from
   extrema_reference.roots_unit (with its horner), the values from its eval_vec.
2. `sample_gate`: a dense sampler in numpy.longdouble in PHYSICAL time, straight from C and T with the flatness map of tests/check_reference.py (h = a + g e3,
   zB, yB, xB).  No normalised time, no polynomial of the plane distance, no root finder: it shares nothing with (1) but the definitions.

`variant` plants an error into (1) for the tests that show the crafted states would catch it:
  "keep_tau0"       the root at tau == 0 of a later piece is kept: a knot on the plane is counted twice
  "best_not_first"  among passing crossings the largest margin is reported in place of the first passage
  "no_reach"        the margin without the body's reach
  "ge_order"        (flags_of) ORDER is set on <, not on <=
"""
import math

import numpy as np

from extrema_reference import eval_vec, roots_unit

FIELDS = ("n_cross", "n_pass", "margin", "time", "piece", "u", "v", "reach_u", "reach_v", "normal_speed")
N_CROSS, N_PASS, MARGIN, TIME, PIECE, U, V, REACH_U, REACH_V, NORMAL_SPEED = range(10)
FLAG_MISSED, FLAG_REPEAT, FLAG_ORDER, FLAG_NONFINITE = 1, 2, 4, 8
NAN = float("nan")
C_NAN, C_PASS, C_MISS = 0, 1, 2


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _sqrt(x):
    return math.sqrt(x) if x >= 0.0 else NAN


def _div(a, b):
    """IEEE division (Python raises where IEEE returns inf / NaN)"""
    if b == 0.0:
        if a == 0.0 or a != a:
            return NAN
        return math.copysign(math.inf, a) * math.copysign(1.0, b)
    return a / b


def gate_frame(rec):
    """(ok, c, wu, wv, eu, ev, n) of a record {c, a, b}"""
    rec = [float(x) for x in np.asarray(rec, dtype=np.float64).reshape(9)]
    c, a, b = rec[0:3], rec[3:6], rec[6:9]
    ok = all(math.isfinite(x) for x in rec)
    if not ok:
        return False, c, NAN, NAN, None, None, None
    wu, wv = _sqrt(_dot(a, a)), _sqrt(_dot(b, b))
    m = [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]
    mn = _sqrt(_dot(m, m))
    if wu == 0.0 or wv == 0.0 or mn == 0.0:
        return False, c, wu, wv, None, None, None
    return True, c, wu, wv, [x / wu for x in a], [x / wv for x in b], [x / mn for x in m]


def _reach(ell, xB, yB1, yB2, zB, e):
    p0, p1, p2 = ell[0] * _dot(xB, e), ell[1] * (yB1 * e[1] + yB2 * e[2]), ell[2] * _dot(zB, e)
    return _sqrt(p0 * p0 + p1 * p1 + p2 * p2)


def _before(k1, k2):
    """the order of the reported crossing on keys (class, margin, index)"""
    if k1[0] != k2[0]:
        return k1[0] < k2[0]
    if k1[0] == C_MISS and k1[1] != k2[1]:
        return k1[1] > k2[1]
    return k1[2] < k2[2]


def gate_row(T, Cp, rec, ell, g, variant=None):
    """The ten fields of one (candidate, gate).  T: (N,) durations, Cp: (N, 6, 3) coefficients of the candidate's pieces, rec: the gate's 9 doubles."""
    T = [float(t) for t in np.asarray(T, dtype=np.float64).reshape(-1)]
    Cp = np.asarray(Cp, dtype=np.float64).reshape(-1, 6, 3)
    ok, c, wu, wv, eu, ev, n = gate_frame(rec)
    if not ok or not all(math.isfinite(t) and t > 0.0 for t in T) or not np.isfinite(Cp).all():
        return np.full(10, np.nan)
    ncross = npass = 0
    best = None
    for k, h in enumerate(T):
        w = [[float(x) for x in row] for row in Cp[k]]
        hp = h
        for j in range(1, 6):
            w[j] = [w[j][d] * hp for d in range(3)]
            hp *= h
        d0 = [w[0][d] - c[d] for d in range(3)]
        f = [_dot(n, w[j]) for j in range(5, 0, -1)] + [_dot(n, d0)]       # highest power first
        roots = roots_unit(f, 5)
        if not roots:
            continue
        wv1 = [[float(j + 1) * w[j + 1][d] for d in range(3)] for j in range(5)]
        wa = [[float((j + 2) * (j + 1)) * w[j + 2][d] for d in range(3)] for j in range(4)]
        for q, tau in enumerate(roots):
            if tau == 0.0 and k != 0 and variant != "keep_tau0":
                continue
            pos, vel, acc = eval_vec(w, 5, tau), eval_vec(wv1, 4, tau), eval_vec(wa, 3, tau)
            hh = h * h
            vel = [x / h for x in vel]
            acc = [x / hh for x in acc]
            th = [acc[0], acc[1], acc[2] + g]
            tn = _sqrt(_dot(th, th))
            zB = [_div(x, tn) for x in th]
            yn = _sqrt(zB[2] * zB[2] + zB[1] * zB[1])
            yB1, yB2 = _div(zB[2], yn), _div(-zB[1], yn)
            xB = [yB1 * zB[2] - yB2 * zB[1], yB2 * zB[0], -(yB1 * zB[0])]
            dc = [pos[d] - c[d] for d in range(3)]
            s, t = _dot(eu, dc), _dot(ev, dc)
            ru, rv = _reach(ell, xB, yB1, yB2, zB, eu), _reach(ell, xB, yB1, yB2, zB, ev)
            if variant == "no_reach":
                mu, mv = wu - abs(s), wv - abs(t)
            else:
                mu, mv = (wu - abs(s)) - ru, (wv - abs(t)) - rv
            margin = mu if (mu != mu or mu <= mv) else mv
            cls = C_NAN if margin != margin else (C_PASS if margin >= 0.0 else C_MISS)
            ncross += 1
            npass += cls == C_PASS
            key = (cls, margin, 8 * k + q)
            if variant == "best_not_first" and cls == C_PASS:
                key = (cls, margin, -margin)
            if best is None or _before(key, best[0]):
                best = (key, [margin, tau, h, k, s, t, ru, rv, _dot(n, vel)])
    if best is None:
        return np.array([0.0, 0.0, -math.inf, 0.0, -1.0, 0.0, 0.0, 0.0, 0.0, 0.0])
    margin, tau, h, k, s, t, ru, rv, ns = best[1]
    cum = 0.0
    for i in range(k):
        cum += T[i]
    return np.array([float(ncross), float(npass), margin, cum + tau * h, float(k), s, t, ru, rv, ns])


def rows(T, Cf, piece_off, gates, gate_off, ell, g, variant=None):
    """Gate rows (n_gates, 10) of a batch: candidate b owns the pieces piece_off[b] .. piece_off[b + 1] - 1 and the gates gate_off[b] .. gate_off[b + 1] - 1"""
    T = np.asarray(T, dtype=np.float64)
    Cp = np.asarray(Cf, dtype=np.float64).reshape(-1, 6, 3)
    gates = np.asarray(gates, dtype=np.float64).reshape(-1, 9)
    out = []
    with np.errstate(all="ignore"):
        for b in range(len(piece_off) - 1):
            sl = slice(int(piece_off[b]), int(piece_off[b + 1]))
            for gi in range(int(gate_off[b]), int(gate_off[b + 1])):
                out.append(gate_row(T[sl], Cp[sl], gates[gi], ell, g, variant))
    return np.array(out).reshape(-1, 10)


def flags_of(grows, gate_off, variant=None):
    """FRX_GATE_FLAG_* bits per candidate"""
    grows = np.asarray(grows, dtype=np.float64).reshape(-1, 10)
    out = np.zeros(len(gate_off) - 1, np.uint32)
    for b in range(len(gate_off) - 1):
        f, last = 0, -math.inf
        for r in grows[int(gate_off[b]):int(gate_off[b + 1])]:
            if r[N_PASS] == 0.0:
                f |= FLAG_MISSED
            if r[N_PASS] > 1.0:
                f |= FLAG_REPEAT
            if r[N_PASS] > 0.0:
                if (r[TIME] < last) if variant == "ge_order" else (not r[TIME] > last):
                    f |= FLAG_ORDER
                last = r[TIME]
            if np.isnan(r).any():
                f |= FLAG_NONFINITE
        out[b] = f
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the independent sampler: long double, physical time, the flatness map as tests/check_reference.py writes it
# ---------------------------------------------------------------------------------------------------------------------
L = np.longdouble


def _frame_ld(rec):
    rec = np.asarray(rec, dtype=np.float64).reshape(9).astype(L)
    c, a, b = rec[0:3], rec[3:6], rec[6:9]
    wu, wv = np.sqrt((a * a).sum()), np.sqrt((b * b).sum())
    m = np.cross(a, b)
    return c, wu, wv, a / wu, b / wv, m / np.sqrt((m * m).sum())


def sample_values(c6, t, rec, ell, g, only_f=False):
    """Everything the row reports, by its definition, of one piece at the physical times t (numpy.longdouble arrays): plane distance f = n.(p - c),
    u, v, reach_u, reach_v, margin, normal_speed"""
    c6 = np.asarray(c6, dtype=np.float64).reshape(6, 3).astype(L)
    s = np.asarray(t, dtype=L).reshape(-1)
    one, z = np.ones_like(s), np.zeros_like(s)
    beta0 = np.stack([one, s, s ** 2, s ** 3, s ** 4, s ** 5], axis=1)
    beta1 = np.stack([z, one, 2 * s, 3 * s ** 2, 4 * s ** 3, 5 * s ** 4], axis=1)
    beta2 = np.stack([z, z, 2 * one, 6 * s, 12 * s ** 2, 20 * s ** 3], axis=1)
    pos, vel, acc = beta0 @ c6, beta1 @ c6, beta2 @ c6
    gc, wu, wv, eu, ev, n = _frame_ld(rec)
    if only_f:
        return dict(f=(pos - gc) @ n)
    h = acc.copy()
    h[:, 2] += L(g)
    E = np.asarray(ell, dtype=np.float64).astype(L)
    with np.errstate(all="ignore"):
        zB = h / np.sqrt((h * h).sum(axis=1))[:, None]
        czB = np.stack([z, zB[:, 2], -zB[:, 1]], axis=1)
        yB = czB / np.sqrt((czB * czB).sum(axis=1))[:, None]
        xB = np.cross(yB, zB)
        R = np.stack([xB, yB, zB], axis=2)                               # columns xB, yB, zB
        d = pos - gc
        u, v = d @ eu, d @ ev
        ru = np.sqrt((((R.transpose(0, 2, 1) @ eu) * E) ** 2).sum(axis=1))   # |E R^T eu|
        rv = np.sqrt((((R.transpose(0, 2, 1) @ ev) * E) ** 2).sum(axis=1))
        return dict(f=d @ n, u=u, v=v, reach_u=ru, reach_v=rv, margin=np.minimum(wu - np.abs(u) - ru, wv - np.abs(v) - rv), normal_speed=vel @ n)


def scale(c6, T, rec):
    """S = |c| + sum_k |c_k| T^k: the size every bound on n.(p - c) is relative to"""
    c6 = np.asarray(c6, dtype=np.float64).reshape(6, 3)
    return float(np.linalg.norm(np.asarray(rec, dtype=np.float64)[:3]) + sum(np.linalg.norm(c6[k]) * float(T) ** k for k in range(6)))


def sample_gate(T, Cp, rec, ell, g, n=20001):
    """The sampler's view of one (candidate, gate): dict(n_cross = sign changes of f over n samples of every piece, counted once per candidate (a knot sample that is
    exactly zero belongs to the earlier piece), doubtful = the sampler itself sees a near-tangency (a local extremum sample of f with |f| < 1e-9 S) or a
    root within two sample steps of a piece end)"""
    T = np.asarray(T, dtype=np.float64).reshape(-1)
    Cp = np.asarray(Cp, dtype=np.float64).reshape(-1, 6, 3)
    ncross, doubtful = 0, False
    for k in range(len(T)):
        t = np.linspace(L(0), L(T[k]), n)
        f = sample_values(Cp[k], t, rec, ell, g, only_f=True)["f"]
        S = scale(Cp[k], T[k], rec)
        sg = np.sign(f)
        nz = np.flatnonzero(sg != 0)
        if len(nz) == 0:
            doubtful = True
            continue
        change = np.flatnonzero(sg[nz][1:] != sg[nz][:-1])               # between the non-zero samples nz[i] and nz[i + 1]
        ncross += len(change)
        if len(nz) != n:
            doubtful = True                                              # an exact zero among the samples: a root on a sample (ends included)
        for i in change:
            if nz[i] < 2 or nz[i + 1] > n - 3:
                doubtful = True
        af = np.abs(f)
        ext = (af[1:-1] <= af[:-2]) & (af[1:-1] <= af[2:]) & (sg[1:-1] == sg[:-2]) & (sg[1:-1] == sg[2:])   # |f| dips without a sign change
        if (af[1:-1][ext] < 1e-9 * S).any() or min(af[0], af[1], af[2], af[-1], af[-2], af[-3]) < 1e-9 * S:
            doubtful = True
    return dict(n_cross=ncross, doubtful=doubtful)


def field_failures(row, T, Cp, rec, ell, g):
    """The issue's comparison of one row that reports a crossing with the sampler's formulas at the reported TIME: |n.(p - c)| <= 256 eps S there, every other
    field to 1e-9 max(1, |value|).  Returns the list of what fails."""
    T = np.asarray(T, dtype=np.float64).reshape(-1)
    Cp = np.asarray(Cp, dtype=np.float64).reshape(-1, 6, 3)
    k = int(row[PIECE])
    cum = L(0)
    for i in range(k):
        cum += L(T[i])
    tl = L(row[TIME]) - cum
    v = sample_values(Cp[k], [tl], rec, ell, g)
    S = scale(Cp[k], T[k], rec)
    bad = []
    if not (-1e-12 <= float(tl) <= T[k] * (1 + 1e-12)):
        bad.append(("local time", float(tl), float(T[k])))
    if not abs(float(v["f"][0])) <= 256 * np.finfo(np.float64).eps * S:
        bad.append(("plane", float(v["f"][0]), S))
    for name, fi in (("margin", MARGIN), ("u", U), ("v", V), ("reach_u", REACH_U), ("reach_v", REACH_V), ("normal_speed", NORMAL_SPEED)):
        want = float(v[name][0])
        if not ((want != want and row[fi] != row[fi]) or abs(row[fi] - want) <= 1e-9 * max(1.0, abs(want))):
            bad.append((name, float(row[fi]), want))
    return bad


def expectation_failures(row, expect, tol=1e-9):
    """deviations of a row from a crafted state's closed-form values: expect maps a field name to a value (compared to tol max(1, |value|); an int or
    +-inf exactly) or to a (value, tol) pair"""
    bad = []
    for name, val in expect.items():
        t = tol
        if isinstance(val, tuple):
            val, t = val
        got = row[FIELDS.index(name)]
        if isinstance(val, int) or math.isinf(val):
            ok = got == val
        else:
            ok = (val != val and got != got) or abs(got - val) <= t * max(1.0, abs(val))
        if not ok:
            bad.append((name, float(got), val))
    return bad
