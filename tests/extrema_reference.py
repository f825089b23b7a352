"""Restatement of the exact per-piece extrema (frx_trajectory_extrema, include/frx.h) - test infrastructure, not a test module.

Two independent things live here.

1. `piece_row` / `rows`: the kernel's arithmetic restated operation by operation in float64 (Python floats: every + - * / is one correctly rounded IEEE
   operation, nothing is fused; math.sqrt is correctly rounded).  It is the referee for bit identity.  `roots_unit` is the recursion of frx_geometry.cpp as
   it stands, leading-zero strip, degree-1 base case and the three zero tests included.
2. `sample_piece`: a dense sampler in numpy.longdouble in PHYSICAL time, straight from C and T with the flatness map of tests/check_reference.py (h = a + g e3,
   zB, yB, xB, omega_xy = (xB.j, yB.j) / |h|).  No normalised time, no polynomial of a norm: it shares nothing with (1) but the definitions.

`variant` plants an error into (1) for the tests that show the sampler comparison would catch it:
  "no_end"    tau = 1 is not a candidate          "drop_fa"  a root found by fa == 0 is dropped
  "ge"        a later candidate replaces on >= / <=      "min_first"  the minimum is the value of the first candidate
"""
import math

import numpy as np

FIELDS = ("speed", "acc", "thrust_min", "thrust_max", "body_rate", "t_speed", "t_acc", "t_thrust_min", "t_thrust_max", "t_body_rate")
NAN = float("nan")


def horner(c, deg, x):
    v = c[0]
    for i in range(1, deg + 1):
        v = v * x + c[i]
    return v


def roots_unit(c, deg, variant=None):
    """all sign-change roots of c (highest power first, degree deg) in [0, 1], ascending"""
    c = list(c)
    while deg > 0 and c[0] == 0.0:
        c = c[1:]
        deg -= 1
    if deg <= 0:
        return []
    if deg == 1:
        r = -c[1] / c[0]
        return [r] if (r >= 0.0 and r <= 1.0) else []
    dc = [c[i] * float(deg - i) for i in range(deg)]
    pts = [0.0] + roots_unit(dc, deg - 1, variant) + [1.0]
    out = []
    for i in range(len(pts) - 1):
        a, b = pts[i], pts[i + 1]
        fa, fb = horner(c, deg, a), horner(c, deg, b)
        if fa == 0.0:
            if variant != "drop_fa" and (not out or out[-1] != a):
                out.append(a)
            continue
        if fb == 0.0:
            out.append(b)
            continue
        if (fa < 0.0) == (fb < 0.0):
            continue
        it = 0
        while it < 200 and b - a > 0.0:
            m = 0.5 * (a + b)
            if m <= a or m >= b:
                break
            fm = horner(c, deg, m)
            if fm == 0.0:
                a = b = m
                break
            if (fm < 0.0) == (fa < 0.0):
                a, fa = m, fm
            else:
                b = m
            it += 1
        out.append(0.5 * (a + b))
    return out


def sq_norm(w, deg):
    """|w|^2, lowest power first, by the host's i-outer, j-inner double loop"""
    sq = [0.0] * (2 * deg + 1)
    for i in range(deg + 1):
        for j in range(deg + 1):
            sq[i + j] += w[i][0] * w[j][0] + w[i][1] * w[j][1] + w[i][2] * w[j][2]
    return sq


def eval_vec(w, deg, t):
    v = [0.0, 0.0, 0.0]
    tn = 1.0
    for k in range(deg + 1):
        v[0] += w[k][0] * tn
        v[1] += w[k][1] * tn
        v[2] += w[k][2] * tn
        tn *= t
    return v


class Best:
    """running extremum over the candidates in their order: strict > (<), the first candidate wins a tie, a NaN takes the field and stays"""

    def __init__(self, sign, variant=None):
        self.sign, self.any, self.v, self.t, self.variant = sign, False, NAN, NAN, variant

    def take(self, x, tau):
        if self.variant == "min_first" and self.sign < 0 and self.any:
            return
        if not self.any:
            rep = True
        elif self.v != self.v:
            rep = False
        elif x != x:
            rep = True
        elif self.variant == "ge":
            rep = x >= self.v if self.sign > 0 else x <= self.v
        else:
            rep = x > self.v if self.sign > 0 else x < self.v
        if rep:
            self.v, self.t = x, tau
        self.any = True


def candidates(top, deg, variant):
    cand = roots_unit(top, deg, variant) + [0.0]
    if variant != "no_end":
        cand.append(1.0)
    return cand


def norm_task(w, deg, variant, want_min=False):
    sq = sq_norm(w, deg)
    d2 = 2 * deg
    der = [float(k) * sq[k] for k in range(d2, 0, -1)]                   # derivative, highest power first
    hi, lo = Best(+1, variant), Best(-1, variant)
    for tau in candidates(der, d2 - 1, variant):
        v = eval_vec(w, deg, tau)
        val = v[0] * v[0] + v[1] * v[1] + v[2] * v[2]
        hi.take(val, tau)
        if want_min:
            lo.take(val, tau)
    return hi, lo


def rate_task(wh, variant):
    wj = [[float(k + 1) * wh[k + 1][d] for d in range(3)] for k in range(3)]
    X = [[0.0, 0.0, 0.0] for _ in range(5)]
    for i in range(4):
        for k in range(3):
            if i + k <= 4:
                X[i + k][0] += wh[i][1] * wj[k][2] - wh[i][2] * wj[k][1]
                X[i + k][1] += wh[i][2] * wj[k][0] - wh[i][0] * wj[k][2]
                X[i + k][2] += wh[i][0] * wj[k][1] - wh[i][1] * wj[k][0]
    N, Q = sq_norm(X, 4), sq_norm(wh, 3)
    Np = [float(k + 1) * N[k + 1] for k in range(8)]
    Qp = [float(k + 1) * Q[k + 1] for k in range(6)]
    A, B = [0.0] * 14, [0.0] * 14
    for i in range(8):
        for j in range(7):
            A[i + j] += Np[i] * Q[j]
    for i in range(9):
        for j in range(6):
            B[i + j] += N[i] * Qp[j]
    top = [A[m] - 2.0 * B[m] for m in range(13, -1, -1)]
    hi = Best(+1, variant)
    for tau in candidates(top, 13, variant):
        hv, jv = eval_vec(wh, 3, tau), eval_vec(wj, 2, tau)
        x0 = hv[1] * jv[2] - hv[2] * jv[1]
        x1 = hv[2] * jv[0] - hv[0] * jv[2]
        x2 = hv[0] * jv[1] - hv[1] * jv[0]
        nv = x0 * x0 + x1 * x1 + x2 * x2
        qv = hv[0] * hv[0] + hv[1] * hv[1] + hv[2] * hv[2]
        qq = qv * qv
        hi.take(nv / qq if qq != 0.0 else (NAN if nv == 0.0 or nv != nv else math.copysign(math.inf, nv)), tau)
    return hi


def host_derivative_norms(c, T):
    """dn of frx_traj_max_rates' max_sq_norm for |v| and |a| (it returns 0 when dn < 2.22e-16: the inputs of a bit comparison must stay clear of that)"""
    c = [[float(x) for x in row] for row in np.asarray(c, dtype=np.float64).reshape(6, 3)]
    h = float(T)
    wv, hp = [], h
    for k in range(5):
        wv.append([float(k + 1) * c[k + 1][d] * hp for d in range(3)])
        hp *= h
    wa, hp = [], h * h
    for k in range(4):
        wa.append([float((k + 2) * (k + 1)) * c[k + 2][d] * hp for d in range(3)])
        hp *= h
    out = []
    for w, deg in ((wv, 4), (wa, 3)):
        sq = sq_norm(w, deg)
        out.append(sum((float(k) * sq[k]) ** 2 for k in range(2 * deg, 0, -1)))
    return out


def _sqrt(x):
    return math.sqrt(x) if x >= 0.0 else NAN                              # (NaN in, NaN out; a squared norm is never negative)


def piece_row(c, T, g, variant=None):
    """The ten fields of one piece.  c: (6, 3) coefficients (row k = power k)."""
    c = [[float(x) for x in row] for row in np.asarray(c, dtype=np.float64).reshape(6, 3)]
    h = float(T)
    if not (math.isfinite(h) and h > 0.0) or not all(math.isfinite(x) for row in c for x in row):
        return np.full(10, np.nan)
    with np.errstate(all="ignore"):
        wv, hp = [], h
        for k in range(5):
            wv.append([float(k + 1) * c[k + 1][d] * hp for d in range(3)])
            hp *= h
        wa, hp = [], h * h
        for k in range(4):
            wa.append([float((k + 2) * (k + 1)) * c[k + 2][d] * hp for d in range(3)])
            hp *= h
        wh = [list(r) for r in wa]
        wh[0][2] = wh[0][2] + g * (h * h)
        sp, _ = norm_task(wv, 4, variant)
        ac, _ = norm_task(wa, 3, variant)
        th, tl = norm_task(wh, 3, variant, want_min=True)
        br = rate_task(wh, variant)
    return np.array([_sqrt(sp.v) / h, _sqrt(ac.v) / (h * h), _sqrt(tl.v) / (h * h), _sqrt(th.v) / (h * h), _sqrt(br.v) / h,
                     sp.t * h, ac.t * h, tl.t * h, th.t * h, br.t * h])


def rows(T, Cf, g, variant=None):
    Cp = np.asarray(Cf, dtype=np.float64).reshape(-1, 6, 3)
    return np.array([piece_row(Cp[i], float(T[i]), g, variant) for i in range(len(T))])


def reduce_candidates(prow, T, piece_off):
    """Candidate rows (B, 10): per field, in piece order, strict > (< for thrust_min), first piece wins a tie, NaN propagates; times from the
    candidate's start on prefix sums taken left to right."""
    out = []
    for b in range(len(piece_off) - 1):
        o = np.empty(10)
        t0 = 0.0
        for gp in range(piece_off[b], piece_off[b + 1]):
            r = prow[gp]
            for f in range(5):
                a, cc = o[f], r[f]
                better = cc < a if f == 2 else cc > a
                if gp == piece_off[b] or (a == a and (better or cc != cc)):
                    o[f] = cc
                    o[5 + f] = t0 + r[5 + f]
            t0 += float(T[gp])
        out.append(o)
    return np.array(out)


def flags_of(cand, params):
    """FRX_CHECK_FLAG_* bits per candidate, no slack (there is no corridor bit here)"""
    f = np.zeros(len(cand), np.uint32)
    with np.errstate(invalid="ignore"):
        f |= np.where(cand[:, 0] > params["vel_max"], 2, 0).astype(np.uint32)
        f |= np.where(cand[:, 2] < params["thr_acc_min"], 4, 0).astype(np.uint32)
        f |= np.where(cand[:, 3] > params["thr_acc_max"], 8, 0).astype(np.uint32)
        f |= np.where(cand[:, 4] > params["body_rate_max"], 16, 0).astype(np.uint32)
        f |= np.where(~np.isfinite(cand).all(axis=1), 32, 0).astype(np.uint32)
    return f


# ---------------------------------------------------------------------------------------------------------------------
# the independent sampler: long double, physical time, the flatness map as tests/check_reference.py writes it
# ---------------------------------------------------------------------------------------------------------------------
def sample_values(c, t, g):
    """speed, acc, thrust, body_rate (numpy.longdouble arrays) of one piece at the physical times t"""
    L = np.longdouble
    c = np.asarray(c, dtype=np.float64).reshape(6, 3).astype(L)
    s = np.asarray(t, dtype=L).reshape(-1)
    one, z = np.ones_like(s), np.zeros_like(s)
    beta1 = np.stack([z, one, 2 * s, 3 * s ** 2, 4 * s ** 3, 5 * s ** 4], axis=1)
    beta2 = np.stack([z, z, 2 * one, 6 * s, 12 * s ** 2, 20 * s ** 3], axis=1)
    beta3 = np.stack([z, z, z, 6 * one, 24 * s, 60 * s ** 2], axis=1)
    vel, acc, jer = beta1 @ c, beta2 @ c, beta3 @ c
    h = acc.copy()
    h[:, 2] += L(g)
    with np.errstate(all="ignore"):
        fThr = np.sqrt((h * h).sum(axis=1))
        zB = h / fThr[:, None]
        czB = np.stack([z, zB[:, 2], -zB[:, 1]], axis=1)
        yB = czB / np.sqrt((czB * czB).sum(axis=1))[:, None]
        xB = np.cross(yB, zB)
        b0 = (xB * jer).sum(axis=1) / fThr
        b1 = (yB * jer).sum(axis=1) / fThr
        return dict(speed=np.sqrt((vel * vel).sum(axis=1)), acc=np.sqrt((acc * acc).sum(axis=1)), thrust=fThr, body_rate=np.sqrt(b0 * b0 + b1 * b1))


def sample_piece(c, T, g, n=20001):
    """max speed, max acc, min thrust, max thrust, max body rate over n samples of [0, T] (float64 of the long-double values)"""
    t = np.linspace(np.longdouble(0), np.longdouble(T), n)
    v = sample_values(c, t, g)
    return np.array([v["speed"].max(), v["acc"].max(), v["thrust"].min(), v["thrust"].max(), v["body_rate"].max()], dtype=np.float64)


KEYS = ("speed", "acc", "thrust", "thrust", "body_rate")


def bound_failures(row, c, T, g, n=20001):
    """The issue's comparison of one restatement (or device) row with the sampler; returns the list of what fails (empty: passes).
    max >= sampled (1 - 1e-12) and <= sampled (1 + 1e-6) + 1e-12, mirrored for the minimum; every reported time reproduces its value to 1e-9."""
    s = sample_piece(c, T, g, n)
    bad = []
    for f in range(5):
        v = row[f]
        if v != v or s[f] != s[f]:
            ok = v != v and s[f] != s[f]                                   # (h = 0: not a number on both sides)
        elif f == 2:
            ok = v <= s[f] * (1 + 1e-12) and v >= s[f] * (1 - 1e-6) - 1e-12
        else:
            ok = v >= s[f] * (1 - 1e-12) and v <= s[f] * (1 + 1e-6) + 1e-12
        if not ok:
            bad.append((FIELDS[f], float(v), float(s[f])))
        at = float(sample_values(c, [row[5 + f]], g)[KEYS[f]][0])
        if not (0.0 <= row[5 + f] <= T and ((at != at and v != v) or abs(at - v) <= 1e-9 * max(1.0, abs(v)))):
            bad.append((FIELDS[5 + f], float(row[5 + f]), at, float(v)))
    return bad


def expectation_failures(row, expect, tol=1e-9):
    """deviations of a row from a crafted state's closed-form (value, time) pairs (time None: not fixed by the state)"""
    bad = []
    for name, (val, t) in expect.items():
        f = FIELDS.index(name)
        if not ((val != val and row[f] != row[f]) or abs(row[f] - val) <= tol * max(1.0, abs(val))):
            bad.append((name, float(row[f]), val))
        if t is not None and not abs(row[5 + f] - t) <= tol:
            bad.append(("t_" + name, float(row[5 + f]), t))
    return bad
