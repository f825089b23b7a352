"""Restatement of the exact clearance certificate (frx_trajectory_clearance_exact, include/frx.h) - test infrastructure, not a test module.

Two independent things live here.

1. `setup` / `value` / `dist_task` / `ell_task` / `piece_row` / `rows` / `reduce_candidates` / `flags_of`: the kernel's arithmetic restated operation by operation
   in float64 (Python floats: every + - * / is one correctly rounded IEEE operation, nothing is fused; math.sqrt is correctly rounded).  It is the referee for
   bit identity.  The roots come from extrema_reference.roots_unit, the running-power sums from its eval_vec, the candidate rule from its Best.
   The cull is restated by its RULES, not by the kernel's schedule: the box of the Bezier control points, the bounds R_ub / Q_ub from values at candidates
   (tau = 0 and 1 of every point, then the minima found so far), points taken in ascending box distance.  A row must not depend on the schedule - that is what
   the comparison with the device, and with cull=False, checks.  `counts`, when given, receives (survivors, DIST tasks, ELL tasks) of the piece.
2. `sample_min`: a dense sampler in numpy.longdouble in PHYSICAL time, straight from C and T with the flatness map of tests/check_reference.py and the FULL frame
   R = [xB yB zB] of the dense kernel, refined round its best sample by golden section.  No normalised time, no identity for q, no polynomial, no root finder.
"""
import math

import numpy as np

from extrema_reference import Best, eval_vec, roots_unit

FIELDS = ("ell", "dist", "t_ell", "i_ell", "t_dist", "i_dist")
ELL, DIST, T_ELL, I_ELL, T_DIST, I_DIST = range(6)
FLAG_COLLISION, FLAG_NONFINITE = 1, 2
NAN = float("nan")
INFL = 1.0 + 2.0 ** -20
BEZ = [[1.0], [1.0, 0.2], [1.0, 0.4, 0.1], [1.0, 0.6, 0.3, 0.1], [1.0, 0.8, 0.6, 0.4, 0.2], [1.0, 1.0, 1.0, 1.0, 1.0, 1.0]]


def _div(a, b):
    """IEEE division (Python raises where IEEE returns inf / NaN)"""
    if b == 0.0:
        if a == 0.0 or a != a:
            return NAN
        return math.copysign(math.inf, a) * math.copysign(1.0, b)
    return a / b


def _sqrt(x):
    return math.sqrt(x) if x >= 0.0 else NAN


def mul(a, b):
    """out[i + j] += a[i] b[j], i outer, j inner"""
    out = [0.0] * (len(a) + len(b) - 1)
    for i in range(len(a)):
        for j in range(len(b)):
            out[i + j] += a[i] * b[j]
    return out


def before(v1, i1, v2, i2):
    """is (v1, i1) before (v2, i2)?  NaN first, then the smaller value, then the lower point; i None is after everything"""
    if i1 is None:
        return False
    if i2 is None:
        return True
    n1, n2 = v1 != v1, v2 != v2
    if n1 or n2:
        return n1 and (not n2 or i1 < i2)
    return v1 < v2 or (v1 == v2 and i1 < i2)


def setup(T, c, g, eh, ev):
    """what the kernel knows of a valid piece: w_k = c_k T^k, wh = T^2 (a + g e3), Q, Q^2, Q', the widened box, the squared semi-axes"""
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
    Q2 = mul(Q, Q)
    Qp = [float(k + 1) * Q[k + 1] for k in range(6)]
    lo, hi = [0.0] * 3, [0.0] * 3
    for d in range(3):
        l = u = w[0][d]
        s = 0.0
        for j in range(1, 6):
            b = w[0][d]
            for k in range(1, j + 1):
                b += BEZ[j][k] * w[k][d]
            l = b if b < l else l
            u = b if b > u else u
        for k in range(6):
            s += abs(w[k][d])
        pad = s * 2.0 ** -40
        lo[d], hi[d] = l - pad, u + pad
    eh2, ev2 = eh * eh, ev * ev
    return dict(h=h, w=w, wh=wh, Q=Q, Q2=Q2, Qp=Qp, lo=lo, hi=hi, eh2=eh2, ev2=ev2, delta=ev2 - eh2, emax2=eh2 if eh2 > ev2 else ev2)


def value(pc, o, tau):
    """(r, q) of the point o at tau, directly from p and wh"""
    pos, hv = eval_vec(pc["w"], 5, tau), eval_vec(pc["wh"], 3, tau)
    u = [o[0] - pos[0], o[1] - pos[1], o[2] - pos[2]]
    S = u[0] * u[0] + u[1] * u[1] + u[2] * u[2]
    m = u[0] * hv[0] + u[1] * hv[1] + u[2] * hv[2]
    Qv = hv[0] * hv[0] + hv[1] * hv[1] + hv[2] * hv[2]
    k = _div(m * m, Qv)
    q = (S - k) / pc["eh2"] + k / pc["ev2"]
    if q < 0.0:
        q = 0.0
    return S, q


def box_d2(pc, o):
    d = []
    for a in range(3):
        below, above = pc["lo"][a] - o[a], o[a] - pc["hi"][a]
        d.append(below if below > 0.0 else (above if above > 0.0 else 0.0))
    return d[0] * d[0] + d[1] * d[1] + d[2] * d[2]


def point_polys(pc, o):
    """(U, S', m) of one point: u(tau), the derivative of S = U.U and m = U.wh, lowest power first"""
    w, wh = pc["w"], pc["wh"]
    U = [[o[d] - w[0][d] for d in range(3)]] + [[-w[k][d] for d in range(3)] for k in range(1, 6)]
    S = [0.0] * 11
    for i in range(6):
        for j in range(6):
            S[i + j] += U[i][0] * U[j][0] + U[i][1] * U[j][1] + U[i][2] * U[j][2]
    Sp = [float(k + 1) * S[k + 1] for k in range(10)]
    m = [0.0] * 9
    for i in range(6):
        for j in range(4):
            m[i + j] += U[i][0] * wh[j][0] + U[i][1] * wh[j][1] + U[i][2] * wh[j][2]
    return U, Sp, m


def ell_poly(pc, Sp, m):
    """F, highest power first"""
    mp = [float(k + 1) * m[k + 1] for k in range(8)]
    A = mul(Sp, pc["Q2"])
    B1 = mul(mp, pc["Q"])
    B2 = mul(m, pc["Qp"])
    G = [2.0 * B1[k] - B2[k] for k in range(14)]
    H = mul(m, G)
    return [pc["ev2"] * A[k] - pc["delta"] * H[k] for k in range(21, -1, -1)]


def dist_task(pc, o, Sp):
    """(min r, tau) of one point"""
    best = Best(-1)
    for tau in roots_unit(Sp[::-1], 9) + [0.0, 1.0]:
        best.take(value(pc, o, tau)[0], tau)
    return best.v, best.t


def ell_task(pc, o, Sp, m):
    """(min q, tau) of one point"""
    best = Best(-1)
    for tau in roots_unit(ell_poly(pc, Sp, m), 21) + [0.0, 1.0]:
        best.take(value(pc, o, tau)[1], tau)
    return best.v, best.t


def piece_row(T, c, obs, params, cull=True, counts=None):
    """The six fields of one piece against the cloud obs (n, 3)"""
    h = float(T)
    c = np.asarray(c, dtype=np.float64).reshape(6, 3)
    if not (math.isfinite(h) and h > 0.0) or not np.isfinite(c).all():
        if counts is not None:
            counts[:] = [0, 0, 0]
        return np.full(6, np.nan)
    eh, ev, g = params["horiz_half_len"], params["vert_half_len"], params["grav_acc"]
    pts = [[float(x) for x in o] for o in np.asarray(obs, dtype=np.float64).reshape(-1, 3)]
    with np.errstate(all="ignore"):
        pc = setup(h, c, g, eh, ev)
        finite = [all(math.isfinite(x) for x in o) for o in pts]
        d2 = [box_d2(pc, o) for o in pts]
        r_ub = q_ub = math.inf
        qoff = False                                                      # a finite point has q = NaN at an end: no number bounds min q, the q side is off
        if cull:
            for o, fin in zip(pts, finite):
                for tau in (0.0, 1.0):
                    r, q = value(pc, o, tau)
                    if r < r_ub:
                        r_ub = r
                    if q < q_ub:
                        q_ub = q
                    if q != q and fin:
                        qoff = True
            if qoff:
                q_ub = math.inf
        order = sorted(range(len(pts)), key=lambda i: (finite[i], d2[i], i))      # any order gives the same row; this one bounds early
        bq = br = tq = tr = 0.0
        iq = ir = None
        nsurv = ndist = nell = 0
        for i in order:
            o = pts[i]
            bound = pc["emax2"] * q_ub
            if cull and finite[i] and d2[i] > (r_ub if r_ub > bound else bound) * INFL:
                continue
            nsurv += 1
            U, Sp, m = point_polys(pc, o)
            lb = d2[i]
            if not (cull and finite[i] and d2[i] > r_ub * INFL):
                ndist += 1
                mr, t = dist_task(pc, o, Sp)
                lb = mr
                if before(mr, i, br, ir):
                    br, tr, ir = mr, t, i
                if mr < r_ub:
                    r_ub = mr
            if cull and finite[i] and lb > pc["emax2"] * q_ub * INFL:
                continue
            nell += 1
            mq, t = ell_task(pc, o, Sp, m)
            if before(mq, i, bq, iq):
                bq, tq, iq = mq, t, i
            if mq < q_ub and not qoff:
                q_ub = mq
        if counts is not None:
            counts[:] = [nsurv, ndist, nell]
        return np.array([_sqrt(bq), _sqrt(br), tq * h, float(iq), tr * h, float(ir)])


def rows(T, Cf, obs, params, cull=True, counts=None):
    """Piece rows (P, 6) of a batch; counts: a list that receives [survivors, DIST tasks, ELL tasks] per piece"""
    T = np.asarray(T, dtype=np.float64).reshape(-1)
    Cp = np.asarray(Cf, dtype=np.float64).reshape(-1, 6, 3)
    out = []
    for i in range(len(T)):
        cnt = [0, 0, 0]
        out.append(piece_row(float(T[i]), Cp[i], obs, params, cull, cnt))
        if counts is not None:
            counts.append(cnt)
    return np.array(out).reshape(-1, 6)


def reduce_candidates(prow, T, piece_off):
    """Candidate rows (B, 6): ELL and DIST each under the order (NaN first, then the smaller value, then the earlier piece), with its own time - from the
    candidate's start on the durations summed left to right - and point.  A candidate without pieces keeps a row of zeros."""
    out = []
    for b in range(len(piece_off) - 1):
        o = np.zeros(6)
        t0 = 0.0
        for gp in range(int(piece_off[b]), int(piece_off[b + 1])):
            r, k = prow[gp], gp - int(piece_off[b])
            for v, t, i in ((ELL, T_ELL, I_ELL), (DIST, T_DIST, I_DIST)):
                if k == 0 or (o[v] == o[v] and (r[v] < o[v] or r[v] != r[v])):
                    o[v], o[t], o[i] = r[v], t0 + r[t], r[i]
            t0 += float(T[gp])
        out.append(o)
    return np.array(out).reshape(-1, 6)


def flags_of(cand, piece_off=None):
    """FRX_CLEAR_FLAG_COLLISION when ELL < 1, _NONFINITE when a field is not finite; a candidate without pieces (piece_off given) has no flags"""
    cand = np.asarray(cand, dtype=np.float64).reshape(-1, 6)
    f = np.zeros(len(cand), np.uint32)
    with np.errstate(invalid="ignore"):
        f |= np.where(cand[:, ELL] < 1.0, FLAG_COLLISION, 0).astype(np.uint32)
        f |= np.where(~np.isfinite(cand).all(axis=1), FLAG_NONFINITE, 0).astype(np.uint32)
    if piece_off is not None:
        f[np.diff(np.asarray(piece_off, dtype=np.int64)) == 0] = 0
    return f


# ---------------------------------------------------------------------------------------------------------------------
# the independent sampler: long double, physical time, the full frame of the dense kernel
# ---------------------------------------------------------------------------------------------------------------------
L = np.longdouble


def sample_q_r(c6, t, o, ell, g):
    """(q, r) (numpy.longdouble arrays) of one piece at the physical times t against the point o: q = sum_k (axis_k . u / e_k)^2 with R = [xB yB zB] of
    h = a + g e3, r = u.u"""
    c6 = np.asarray(c6, dtype=np.float64).reshape(6, 3).astype(L)
    s = np.asarray(t, dtype=L).reshape(-1)
    s2 = s * s
    s3 = s2 * s
    pos = [c6[0, a] + c6[1, a] * s + c6[2, a] * s2 + c6[3, a] * s3 + c6[4, a] * (s2 * s2) + c6[5, a] * (s2 * s3) for a in range(3)]
    h = [2 * c6[2, a] + 6 * c6[3, a] * s + 12 * c6[4, a] * s2 + 20 * c6[5, a] * s3 for a in range(3)]
    h[2] = h[2] + L(g)
    o = np.asarray(o, dtype=np.float64).astype(L)
    E = np.asarray(ell, dtype=np.float64).astype(L)
    with np.errstate(all="ignore"):
        hn = np.sqrt(h[0] * h[0] + h[1] * h[1] + h[2] * h[2])
        zB = [h[0] / hn, h[1] / hn, h[2] / hn]
        yn = np.sqrt(zB[2] * zB[2] + zB[1] * zB[1])
        yB = [np.zeros_like(s), zB[2] / yn, -zB[1] / yn]
        xB = [yB[1] * zB[2] - yB[2] * zB[1], yB[2] * zB[0] - yB[0] * zB[2], yB[0] * zB[1] - yB[1] * zB[0]]
        u = [o[a] - pos[a] for a in range(3)]
        comp = [(B[0] * u[0] + B[1] * u[1] + B[2] * u[2]) / E[i] for i, B in enumerate((xB, yB, zB))]
        return comp[0] * comp[0] + comp[1] * comp[1] + comp[2] * comp[2], u[0] * u[0] + u[1] * u[1] + u[2] * u[2]


def sample_min(c6, T, o, ell, g, n=20001):
    """(min q, min r) as floats: the least of n samples over [0, T], each refined by golden section on the two steps round the best sample"""
    t = np.linspace(L(0), L(T), n)
    out = []
    for which in (0, 1):
        f = lambda x: sample_q_r(c6, x, o, ell, g)[which]                 # noqa: E731
        v = f(t)
        j = int(np.argmin(v))
        a, b = t[max(j - 1, 0)], t[min(j + 1, n - 1)]
        gr = (np.sqrt(L(5)) - 1) / 2
        x1, x2 = b - gr * (b - a), a + gr * (b - a)
        f1, f2 = f([x1])[0], f([x2])[0]
        best = v[j]
        for _ in range(90):
            if f1 < f2:
                b, x2, f2 = x2, x1, f1
                x1 = b - gr * (b - a)
                f1 = f([x1])[0]
            else:
                a, x1, f1 = x1, x2, f2
                x2 = a + gr * (b - a)
                f2 = f([x2])[0]
            best = min(best, f1, f2)
        out.append(float(best))
    return out[0], out[1]
