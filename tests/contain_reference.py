"""Restatement of the exact corridor containment certificate (frx_trajectory_contain, include/frx.h) - test infrastructure, not a test module.

Two independent things live here.

1. `face_result` / `piece_row` / `rows` / `reduce_candidates` / `flags_of`: the kernel's arithmetic restated operation by operation in float64 (Python floats:
   every + - * / is one correctly rounded IEEE operation, nothing is fused; math.sqrt is correctly rounded).  It is the referee for bit identity.  The roots come
   from extrema_reference.roots_unit (with its horner), the running-power sums from its eval_vec, the candidate rule from its Best.  `face_records` restates how
   a handle turns the columns (outer normal, point) of an H-polytope into its records {unit normal, n.(p_k - origin) - safe_margin}.
2. `sample_sd` / `sample_pair`: a dense sampler in numpy.longdouble in PHYSICAL time, straight from C and T with the flatness map of tests/check_reference.py and the
   reach |E R^T n| from the full frame R = [xB yB zB].  No normalised time, no identity for the reach, no polynomial, no root finder: it shares nothing with (1)
   but the definitions.

`variant` plants an error into (1) for the tests that show the crafted states would catch it:
  "keep_far"   roots of F with d > 0 (the far side of the ellipsoid) are kept as contacts
  "no_skip"    a face the body cannot reach is not skipped
  "left_end"   an interval is classed by sd at its left end, not at its midpoint
  "keep_tau0"  the root at tau == 0 of a later piece is kept: a knot on a contact is counted twice
"""
import math

import numpy as np

from extrema_reference import Best, eval_vec, horner, roots_unit

FIELDS = ("n_contact", "outside", "t_exit", "t_enter", "k_exit", "centre", "t_centre", "k_centre")
N_CONTACT, OUTSIDE, T_EXIT, T_ENTER, K_EXIT, CENTRE, T_CENTRE, K_CENTRE = range(8)
FLAG_CORRIDOR, FLAG_NONFINITE = 1, 32
NAN = float("nan")


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


def face_records(hpoly, safe_margin):
    """(org, [(n, c)]) of a 6 x K H-polytope (columns: outer normal, point), as the handle lays its records out: org is the first face's point, n the
    normal divided by its norm, c = n.(p_k - org) - safe_margin summed x, y, z"""
    H = np.asarray(hpoly, dtype=np.float64)
    org = [float(H[3, 0]), float(H[4, 0]), float(H[5, 0])]
    recs = []
    for k in range(H.shape[1]):
        r = [float(x) for x in H[:, k]]
        nn = math.sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2])
        n = [r[0] / nn, r[1] / nn, r[2] / nn]
        recs.append((n, n[0] * (r[3] - org[0]) + n[1] * (r[4] - org[1]) + n[2] * (r[5] - org[2]) - safe_margin))
    return org, recs


def _exit_before(t1, k1, t2, k2):
    if k1 is None:
        return False
    if k2 is None:
        return True
    return t1 < t2 or (t1 == t2 and k1 < k2)


def _centre_before(v1, k1, v2, k2):
    if k1 is None:
        return False
    if k2 is None:
        return True
    n1, n2 = v1 != v1, v2 != v2
    if n1 or n2:
        return n1 and (not n2 or k1 < k2)
    return v1 > v2 or (v1 == v2 and k1 < k2)


def normalised(T, c, g):
    """(w (6, 3), wh (4, 3), Q (7)) of one piece: w_k = c_k T^k, wh = T^2 (a + g e3), Q = |wh|^2, lowest power first"""
    h = float(T)
    w = [[float(x) for x in row] for row in np.asarray(c, dtype=np.float64).reshape(6, 3)]
    hp = h
    for i in range(1, 6):
        w[i] = [w[i][d] * hp for d in range(3)]
        hp *= h
    wh = [[float((i + 2) * (i + 1)) * w[i + 2][d] for d in range(3)] for i in range(4)]
    wh[0][2] = wh[0][2] + g * (h * h)
    Q = [0.0] * 7
    for i in range(4):
        for j in range(4):
            Q[i + j] += wh[i][0] * wh[j][0] + wh[i][1] * wh[j][1] + wh[i][2] * wh[j][2]
    return w, wh, Q


def face_poly(w, wh, Q, org, n, c, margin, slack, eh, ev):
    """(d lowest power first, cm, F highest power first) of one face"""
    cm = c + margin
    d0 = [w[0][0] - org[0], w[0][1] - org[1], w[0][2] - org[2]]
    d = [(_dot(n, d0) - cm) + slack] + [_dot(n, w[i]) for i in range(1, 6)]
    eh2 = eh * eh
    delta = ev * ev - eh2
    A = [0.0] * 11
    for i in range(6):
        for j in range(6):
            A[i + j] += d[i] * d[j]
    A[0] = A[0] - eh2
    u = [_dot(n, wh[i]) for i in range(4)]
    U2 = [0.0] * 7
    for i in range(4):
        for j in range(4):
            U2[i + j] += u[i] * u[j]
    F = [0.0] * 17
    for i in range(11):
        for j in range(7):
            F[i + j] += A[i] * Q[j]
    for m in range(7):
        F[m] = F[m] - delta * U2[m]
    return d, cm, F[::-1]


def sd_direct(w, wh, org, n, cm, slack, eh, ev, tau):
    """sd at tau by the direct formula"""
    pos, hv = eval_vec(w, 5, tau), eval_vec(wh, 3, tau)
    pl = [pos[0] - org[0], pos[1] - org[1], pos[2] - org[2]]
    dv = (_dot(n, pl) - cm) + slack
    qv, uv = _dot(hv, hv), _dot(n, hv)
    eh2 = eh * eh
    delta = ev * ev - eh2
    return dv + _sqrt(eh2 + delta * _div(uv * uv, qv))


def face_result(w, wh, Q, h, org, n, c, first, eh, ev, margin, slack, variant=None):
    """One (piece, face): dict(centre (value, tau), skipped, contacts [tau], intervals [(a, b, outside)], outside (time), excursion (a, b) taus or None)"""
    d, cm, F = face_poly(w, wh, Q, org, n, c, margin, slack, eh, ev)
    dh = d[::-1]
    der = [float(i + 1) * d[i + 1] for i in range(4, -1, -1)]
    best = Best(+1)
    for tau in roots_unit(der, 4) + [0.0, 1.0]:
        best.take(horner(dh, 5, tau), tau)
    out = dict(centre=(best.v, best.t), skipped=False, contacts=[], intervals=[], outside=0.0, excursion=None)
    emax = eh if eh > ev else ev
    if best.v + emax < 0.0 and variant != "no_skip":
        out["skipped"] = True
        return out
    a0, acc, have, opened, fe = 0.0, 0.0, False, False, None
    for tau in roots_unit(F, 16) + [None]:
        b = 1.0
        if tau is not None:
            b = tau
            if not horner(dh, 5, b) <= 0.0 and variant != "keep_far":
                continue
            if b == 0.0 and not first and variant != "keep_tau0":
                continue
            out["contacts"].append(b)
        if b > a0:
            sd = sd_direct(w, wh, org, n, cm, slack, eh, ev, a0 if variant == "left_end" else 0.5 * (a0 + b))
            outside = not sd <= 0.0
            out["intervals"].append((a0, b, outside))
            if outside:
                acc += b - a0
                if not have:
                    have, opened, fe = True, True, [a0, b]
                elif opened:
                    fe[1] = b
            else:
                opened = False
        a0 = b
    out["outside"] = acc * h
    out["excursion"] = tuple(fe) if have else None
    return out


def piece_row(T, c, hpoly, first, params, slack, variant=None):
    """The eight fields of one piece.  c: (6, 3) coefficients (row k = power k), hpoly: the 6 x K polytope of the piece, first: is the piece its candidate's first"""
    h = float(T)
    c = np.asarray(c, dtype=np.float64).reshape(6, 3)
    if not (math.isfinite(h) and h > 0.0) or not np.isfinite(c).all():
        return np.full(8, np.nan)
    eh, ev, g, margin = params["horiz_half_len"], params["vert_half_len"], params["grav_acc"], params["safe_margin"]
    org, recs = face_records(hpoly, margin)
    with np.errstate(all="ignore"):
        w, wh, Q = normalised(h, c, g)
        ncon, outside = 0, 0.0
        ex_t, ex_e, ex_k, ce_v, ce_t, ce_k = 0.0, 0.0, None, 0.0, 0.0, None
        for k, (n, cc) in enumerate(recs):
            r = face_result(w, wh, Q, h, org, n, cc, first, eh, ev, margin, slack, variant)
            if _centre_before(r["centre"][0], k, ce_v, ce_k):
                ce_v, ce_t, ce_k = r["centre"][0], r["centre"][1] * h, k
            if r["skipped"]:
                continue
            ncon += len(r["contacts"])
            if r["outside"] > outside:
                outside = r["outside"]
            if r["excursion"] is not None and _exit_before(r["excursion"][0] * h, k, ex_t, ex_k):
                ex_t, ex_e, ex_k = r["excursion"][0] * h, r["excursion"][1] * h, k
    row = [float(ncon), outside, -1.0, -1.0, -1.0, -math.inf, -1.0, -1.0]
    if ex_k is not None:
        row[2:5] = [ex_t, ex_e, float(ex_k)]
    if ce_k is not None:
        row[5:8] = [ce_v, ce_t, float(ce_k)]
    return np.array(row)


def rows(T, Cf, piece_off, polys, params, slack=0.0, variant=None):
    """Piece rows (P, 8) of a batch: polys[i] is the 6 x K polytope of piece i"""
    T = np.asarray(T, dtype=np.float64).reshape(-1)
    Cp = np.asarray(Cf, dtype=np.float64).reshape(-1, 6, 3)
    firsts = set(int(x) for x in piece_off[:-1])
    return np.array([piece_row(float(T[i]), Cp[i], polys[i], i in firsts, params, slack, variant) for i in range(len(T))]).reshape(-1, 8)


def reduce_candidates(prow, T, piece_off):
    """Candidate rows (B, 8): N_CONTACT summed; OUTSIDE and CENTRE maxima in piece order (strict >, a NaN takes the field and stays); the T_EXIT group from the
    first piece whose T_EXIT is not -1; times from the candidate's start on the durations summed left to right; K_EXIT and K_CENTRE the local piece index.
    A candidate without pieces keeps a row of zeros."""
    out = []
    for b in range(len(piece_off) - 1):
        o = np.zeros(8)
        t0 = 0.0
        for gp in range(int(piece_off[b]), int(piece_off[b + 1])):
            r, k = prow[gp], gp - int(piece_off[b])
            o[0] = r[0] if k == 0 else o[0] + r[0]
            if k == 0 or (o[1] == o[1] and (r[1] > o[1] or r[1] != r[1])):
                o[1] = r[1]
            if k == 0:
                o[2:5] = -1.0
            if o[2] == -1.0 and r[2] != -1.0:
                o[2], o[3], o[4] = t0 + r[2], t0 + r[3], float(k)
            if k == 0 or (o[5] == o[5] and (r[5] > o[5] or r[5] != r[5])):
                o[5], o[6], o[7] = r[5], t0 + r[6], float(k)
            t0 += float(T[gp])
        out.append(o)
    return np.array(out).reshape(-1, 8)


def flags_of(cand, piece_off=None):
    """FRX_CHECK_FLAG_CORRIDOR when T_EXIT >= 0, FRX_CHECK_FLAG_NONFINITE when a field is not finite; a candidate without pieces (piece_off given) has no flags"""
    cand = np.asarray(cand, dtype=np.float64).reshape(-1, 8)
    f = np.zeros(len(cand), np.uint32)
    with np.errstate(invalid="ignore"):
        f |= np.where(cand[:, T_EXIT] >= 0.0, FLAG_CORRIDOR, 0).astype(np.uint32)
        f |= np.where(~np.isfinite(cand).all(axis=1), FLAG_NONFINITE, 0).astype(np.uint32)
    if piece_off is not None:
        f[np.diff(np.asarray(piece_off, dtype=np.int64)) == 0] = 0
    return f


# ---------------------------------------------------------------------------------------------------------------------
# the independent sampler: long double, physical time, the flatness map as tests/check_reference.py writes it
# ---------------------------------------------------------------------------------------------------------------------
L = np.longdouble


def sample_sd(c6, t, normal, point, ell, g, slack=0.0):
    """(sd, d) (numpy.longdouble arrays) of one piece at the physical times t against the face through `point` with outer normal `normal` (normalised here):
    d = n.(p - point) + slack, sd = d + |E R^T n| with R = [xB yB zB] of h = a + g e3"""
    c6 = np.asarray(c6, dtype=np.float64).reshape(6, 3).astype(L)
    s = np.asarray(t, dtype=L).reshape(-1)
    s2 = s * s
    s3 = s2 * s
    pos = [c6[0, a] + c6[1, a] * s + c6[2, a] * s2 + c6[3, a] * s3 + c6[4, a] * (s2 * s2) + c6[5, a] * (s2 * s3) for a in range(3)]
    h = [2 * c6[2, a] + 6 * c6[3, a] * s + 12 * c6[4, a] * s2 + 20 * c6[5, a] * s3 for a in range(3)]
    h[2] = h[2] + L(g)
    n = np.asarray(normal, dtype=np.float64).astype(L)
    n = n / np.sqrt((n * n).sum())
    p = np.asarray(point, dtype=np.float64).astype(L)
    E = np.asarray(ell, dtype=np.float64).astype(L)
    with np.errstate(all="ignore"):
        hn = np.sqrt(h[0] * h[0] + h[1] * h[1] + h[2] * h[2])
        zB = [h[0] / hn, h[1] / hn, h[2] / hn]
        yn = np.sqrt(zB[2] * zB[2] + zB[1] * zB[1])
        yB = [np.zeros_like(s), zB[2] / yn, -zB[1] / yn]                  # normalise(0, zB_z, -zB_y)
        xB = [yB[1] * zB[2] - yB[2] * zB[1], yB[2] * zB[0] - yB[0] * zB[2], yB[0] * zB[1] - yB[1] * zB[0]]   # yB x zB
        comp = [E[i] * (B[0] * n[0] + B[1] * n[1] + B[2] * n[2]) for i, B in enumerate((xB, yB, zB))]         # E R^T n, R = [xB yB zB]
        reach = np.sqrt(comp[0] * comp[0] + comp[1] * comp[1] + comp[2] * comp[2])
        d = (pos[0] - p[0]) * n[0] + (pos[1] - p[1]) * n[1] + (pos[2] - p[2]) * n[2] + L(slack)
        return d + reach, d


def scale(c6, T, normal, point, slack=0.0):
    """S = sum_k |d_k|: the size every bound on sd is relative to (d_k the coefficients of d in normalised time)"""
    c6 = np.asarray(c6, dtype=np.float64).reshape(6, 3)
    n = np.asarray(normal, dtype=np.float64)
    n = n / np.linalg.norm(n)
    dk = [float(n @ (c6[0] - np.asarray(point, dtype=np.float64))) + slack] + [float(n @ c6[k]) * float(T) ** k for k in range(1, 6)]
    return float(np.sum(np.abs(dk)))


def sample_pair(c6, T, normal, point, ell, g, slack=0.0, n=20001):
    """The sampler's view of one (piece, face): dict(changes = sign changes of sd over n samples, doubtful = the sampler itself sees a near-tangency (a local
    extremum of |sd| below 1e-6 without a sign change, or a sample that is exactly zero) or a sign change within two steps of an end)"""
    t = np.linspace(L(0), L(T), n)
    sd, _ = sample_sd(c6, t, normal, point, ell, g, slack)
    sg = np.sign(sd)
    doubtful = bool((sg == 0).any() or np.isnan(sd).any())
    change = np.flatnonzero(sg[1:] != sg[:-1])
    for i in change:
        if i < 2 or i + 1 > n - 3:
            doubtful = True
    af = np.abs(sd)
    ext = (af[1:-1] <= af[:-2]) & (af[1:-1] <= af[2:]) & (sg[1:-1] == sg[:-2]) & (sg[1:-1] == sg[2:])
    if (af[1:-1][ext] < 1e-6).any():
        doubtful = True
    return dict(changes=len(change), doubtful=doubtful)


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
