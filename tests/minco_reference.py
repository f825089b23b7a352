"""TEST INFRASTRUCTURE - the MINCO map (tau, xi) -> (T, q) -> c, the jerk objective and its adjoint restated in numpy.longdouble, with a proof of its own accuracy.

Nothing here calls the library or the oracle.  The formulas are those of the reference as oracle/gcopter_oracle.cpp restates them (forwardT / addLayerTGrad,
forwardP / addLayerPGrad, MINCO_S3::generate's rows, getTrajJerkCost, evalTrajCostGrad's adjoint), written in closed form instead of line by line:
  T        three duration layers: soft total time with the C2 map, fixed total time with the C2 map, fixed total time with the exponential map
  q        q_i = V0 + sum_a V_a r_a^2, r = 2 xi / (1 + |xi|^2), on the vertices of the overlap polytopes 1, 3, 5, .. of the Candidate (grid_res = inf: one piece per polytope)
  c        A(T) c = b(q, head, tail): the dense 6N x 6N system in the reference's row order, solved by a partial-pivoting LU in long double with two steps of
           iterative refinement; the residual is evaluated in twice the working precision (error-free products and sums) on the unevaluated sum of the solution
           and its last correction, and has to stay below 1e-15 max|b| (solve())
  J        sum_i integral_0^T_i |jerk|^2, from the general term c_j . c_k j(j-1)(j-2) k(k-1)(k-2) T^(j+k-5) / (j+k-5)
  adjoint  lambda = A^-T dJ/dc, gq_i = lambda[6i+5], gT_i = -lambda . (dA/dT_i) c + |jerk_i(T_i)|^2, chained through the two layers
  P        optionally the reference's speed penalty on top of J (speed_penalty()): the objective that gives the adjoint's linear solve a right-hand side
The working precision is the x87 extended format (64-bit significand, eps = 1.1e-19) wherever numpy.longdouble is that; the tests that use this module say so."""
import numpy as np

LD = np.longdouble
PER_EVAL_TOL = 1e-9                                   # the per-evaluation tolerance of tests/test_gpu_parity.py
LAYERS = ("soft_c2", "fixed_c2", "fixed_exp")        # (rho > 0, c2_diffeo = 1), (rho = 0, total_t, c2_diffeo = 1), (rho = 0, total_t, c2_diffeo = 0)
ASSERTED_FAMILIES = ("even", "ramp", "loguniform", "alternating", "short_first", "short_last", "short_middle", "long_middle")
EXTREME_FAMILY = "isolated_1e-3"
SIZES = (1, 2, 3, 5, 9, 33, 64, 65, 128)             # 0, 1, 2, 3 reduction steps; one wave's worth of knots; each side of 64; the 128-row class
GATES = {1: 0, 2: 0, 3: 0, 5: 0, 9: 1, 33: 8, 64: 16, 65: 16, 128: 32}


def layer_overrides(layer, total_t=None):
    """The settings that select a duration layer, as frx.Problem / Oracle take them."""
    return {} if layer == "soft_c2" else dict(rho=0.0, total_t=float(total_t), c2_diffeo=1 if layer == "fixed_c2" else 0)


# ---- durations ----
def duration_families(N, rng):
    """name -> durations of N pieces.  The asserted families lie in [0.02, 5] (ratio 250); the extreme one puts 1e-3 among 1.0 and needs N >= 3."""
    fam = {"even": np.ones(N), "ramp": np.geomspace(0.02, 5.0, N), "loguniform": np.exp(rng.uniform(np.log(0.02), np.log(5.0), N)),
           "alternating": np.where(np.arange(N) % 2 == 0, 0.02, 5.0)}
    for name, at in (("short_first", 0), ("short_last", N - 1), ("short_middle", N // 2)):
        fam[name] = np.ones(N); fam[name][at] = 0.02
    fam["long_middle"] = np.full(N, 0.05); fam["long_middle"][N // 2] = 5.0
    if N >= 3:
        fam[EXTREME_FAMILY] = np.ones(N); fam[EXTREME_FAMILY][N // 2] = 1e-3
    return fam


def candidates(sc, N):
    """family -> its candidate: one gate perturbation of scenario 0 per family (candidate b of sc.make_batch(0, B, N, GATES[N]) whatever B), all of N pieces."""
    if N not in _candidates:
        names = list(duration_families(N, np.random.default_rng(N)))
        _candidates[N] = dict(zip(names, sc.make_batch(0, len(names), N, GATES[N])))
    return _candidates[N]


_candidates = {}                                     # (building one enumerates the vertices of 2N - 1 polytopes)


def total_time(N):
    """The total time of the fixed-time handles: the even family keeps its 1.0 per piece, the others are rescaled to it (their ratios are what matters)."""
    return float(N)


def family_tau(N, family, layer):
    """The tau block (float64) that gives the family's durations in the layer."""
    T = duration_families(N, np.random.default_rng(N))[family]
    if layer != "soft_c2": T = T * (total_time(N) / T.sum())
    return backward_T(T, layer)


def _c2(t):
    """The C2 map tau -> (e, de/dtau): (tau/2 + 1) tau + 1 for tau > 0, 1 / ((tau/2 - 1) tau + 1) otherwise."""
    t = np.asarray(t, dtype=LD)
    den = (LD(0.5) * t - 1) * t + 1
    pos = t > 0
    return np.where(pos, (LD(0.5) * t + 1) * t + 1, 1 / den), np.where(pos, t + 1, (1 - t) / (den * den))


def _c2_inverse(r):
    r = np.asarray(r, dtype=np.float64)
    return np.where(r > 1.0, np.sqrt(2.0 * np.maximum(r, 1.0) - 1.0) - 1.0, 1.0 - np.sqrt(2.0 / np.minimum(r, 1.0) - 1.0))


def backward_T(T, layer):
    """Durations -> tau (float64, what the library is given): N values in the soft layer, N - 1 in the fixed ones (the last piece takes the rest)."""
    T = np.asarray(T, dtype=np.float64)
    if layer == "soft_c2":
        return _c2_inverse(T)
    r = T[:-1] / T[-1]
    return _c2_inverse(r) if layer == "fixed_c2" else np.log(r)


def forward_T(tau, layer, total_t=None):
    tau = np.asarray(tau, dtype=LD)
    if layer == "soft_c2":
        return _c2(tau)[0]
    e = _c2(tau)[0] if layer == "fixed_c2" else np.exp(tau)
    den = 1 + e.sum()
    return LD(total_t) * np.concatenate([e / den, [1 / den]])


def layer_T_grad(tau, gT, layer, total_t=None):
    """d f / d tau from d f / d T."""
    tau = np.asarray(tau, dtype=LD)
    if layer == "soft_c2":
        return gT * _c2(tau)[1]
    e, de = _c2(tau) if layer == "fixed_c2" else (np.exp(tau), np.exp(tau))
    den = 1 + e.sum()
    # T_i = s e_i / den, T_last = s / den
    return LD(total_t) * de * ((gT[:-1] - gT[-1]) / den - ((gT[:-1] * e).sum() - gT[-1] * e.sum()) / (den * den))


# ---- waypoints ----
def waypoint_vertices(cand):
    """[(V0, edges 3 x k)] of the inner waypoints: polytope 2i + 1 of the Candidate (the overlap of cells i and i + 1), re-based on its first vertex."""
    out = []
    for i in range(cand.coarse_n - 1):
        V = np.asarray(cand.v_polys[2 * i + 1], dtype=LD)
        out.append((V[:, 0].copy(), V[:, 1:] - V[:, :1]))
    return out


def forward_P(xi, verts):
    """xi -> q ((N - 1) x 3)."""
    xi = np.asarray(xi, dtype=LD)
    q = np.zeros((len(verts), 3), dtype=LD); j = 0
    for i, (V0, E) in enumerate(verts):
        k = E.shape[1]; x = xi[j:j + k]; j += k
        r = 2 * x / (1 + (x * x).sum())
        q[i] = V0 + E @ (r * r)
    assert j == len(xi)
    return q


def layer_P_grad(xi, gq, verts):
    xi = np.asarray(xi, dtype=LD)
    g = np.zeros(len(xi), dtype=LD); j = 0
    for i, (V0, E) in enumerate(verts):
        k = E.shape[1]; x = xi[j:j + k]
        n1 = 1 + (x * x).sum()
        r = 2 * x / n1
        gr = 2 * r * (E.T @ gq[i])                               # d f / d r
        g[j:j + k] = 2 * gr / n1 - 4 * x * (gr * x).sum() / (n1 * n1)   # dr_a / dx_b = 2 delta_ab / n1 - 4 x_a x_b / n1^2
        j += k
    return g


# ---- the linear system ----
def _falling(k, d):
    """k (k - 1) .. (k - d + 1)"""
    out = 1
    for m in range(d): out *= k - m
    return out


def _poly_row(T, d, dT=False):
    """Row of the d-th derivative of a quintic at t = T over its six coefficients; dT: the row's derivative with respect to T."""
    row = np.zeros(6, dtype=LD)
    for k in range(d + (1 if dT else 0), 6):
        row[k] = _falling(k, d) * (k - d) * T ** (k - d - 1) if dT else _falling(k, d) * T ** (k - d)
    return row


# rows 6i+3 .. 6i+8 of an inner piece: continuity of jerk and snap, the waypoint, continuity of p, v, a; (derivative order, column of the next piece's -d! entry or None)
_INNER = ((3, 3), (4, 4), (0, None), (0, 0), (1, 1), (2, 2))


def dense_A(T):
    T = np.asarray(T, dtype=LD); N = len(T)
    A = np.zeros((6 * N, 6 * N), dtype=LD)
    A[0, 0] = 1; A[1, 1] = 1; A[2, 2] = 2
    for i in range(N - 1):
        for r, (d, nxt) in enumerate(_INNER):
            A[6 * i + 3 + r, 6 * i:6 * i + 6] = _poly_row(T[i], d)
            if nxt is not None: A[6 * i + 3 + r, 6 * i + 6 + nxt] = -_falling(d, d)
    for d in range(3):
        A[6 * N - 3 + d, 6 * N - 6:] = _poly_row(T[N - 1], d)
    return A


def dA_dT_times_c(T, c):
    """[(rows, (dA/dT_i c)[rows])] per piece: only the rows that carry powers of T_i."""
    T = np.asarray(T, dtype=LD); N = len(T); out = []
    for i in range(N):
        ci = c[6 * i:6 * i + 6]
        if i < N - 1:
            out.append((slice(6 * i + 3, 6 * i + 9), np.stack([_poly_row(T[i], d, dT=True) @ ci for d, _ in _INNER])))
        else:
            out.append((slice(6 * N - 3, 6 * N), np.stack([_poly_row(T[i], d, dT=True) @ ci for d in range(3)])))
    return out


def rhs_b(q, head, tail):
    """head, tail: 3 x 3, columns (p, v, a), as the Candidate holds them."""
    N = len(q) + 1
    b = np.zeros((6 * N, 3), dtype=LD)
    b[0:3] = np.asarray(head, dtype=LD).T
    for i in range(N - 1): b[6 * i + 5] = q[i]
    b[6 * N - 3:] = np.asarray(tail, dtype=LD).T
    return b


class BandLU:
    """Partial-pivoting LU of a matrix of lower bandwidth LBW (dense storage, updates confined to the band) in long double; solves with A and with A^T."""
    LBW, UBW = 6, 6

    def __init__(self, A):
        n = len(A); U = np.array(A, dtype=LD)
        self.n = n; self.piv = np.zeros(n, dtype=np.int64); self.mul = [None] * n
        for k in range(n - 1):
            hi = min(k + self.LBW + 1, n); ce = min(k + self.LBW + self.UBW + 1, n)
            p = k + int(np.argmax(np.abs(U[k:hi, k])))
            self.piv[k] = p
            if p != k: U[[k, p], k:ce] = U[[p, k], k:ce]
            assert U[k, k] != 0, "singular"
            m = U[k + 1:hi, k] / U[k, k]
            U[k + 1:hi, k + 1:ce] -= np.outer(m, U[k, k + 1:ce])
            U[k + 1:hi, k] = 0
            self.mul[k] = m
        self.U = U
        self.w = self.LBW + self.UBW

    def solve(self, b):
        x = np.array(b, dtype=LD); n = self.n
        for k in range(n - 1):
            p = self.piv[k]
            if p != k: x[[k, p]] = x[[p, k]]
            x[k + 1:k + 1 + len(self.mul[k])] -= np.outer(self.mul[k], x[k])
        for k in range(n - 1, -1, -1):
            ce = min(k + self.w + 1, n)
            x[k] = (x[k] - self.U[k, k + 1:ce] @ x[k + 1:ce]) / self.U[k, k]
        return x

    def solve_T(self, y):
        z = np.array(y, dtype=LD); n = self.n
        for k in range(n):
            lo = max(k - self.w, 0)
            z[k] = (z[k] - self.U[lo:k, k] @ z[lo:k]) / self.U[k, k]
        for k in range(n - 2, -1, -1):
            m = self.mul[k]
            z[k] -= m @ z[k + 1:k + 1 + len(m)]
            p = self.piv[k]
            if p != k: z[[k, p]] = z[[p, k]]
        return z


# error-free transformations in the working precision (Dekker / Knuth): a result pair (s, e) is the exact sum or product
_SPLIT = LD(2) ** ((np.finfo(LD).nmant + 2) // 2) + 1


def _two_sum(a, b):
    s = a + b; bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _two_prod(a, b):
    p = a * b
    ca = _SPLIT * a; ah = ca - (ca - a); al = a - ah
    cb = _SPLIT * b; bh = cb - (cb - b); bl = b - bh
    return p, al * bl - (((p - ah * bh) - al * bh) - ah * bl)


def residual2(A, parts, b, transpose=False):
    """b - A (parts[0] + parts[1] + ..) in twice the working precision (compensated dot products, Ogita-Rump-Oishi Dot2), over the band only."""
    n = len(A); w = BandLU.LBW + BandLU.UBW
    M = A.T if transpose else A
    s = np.array(b, dtype=LD); e = np.zeros_like(s)
    for off in range(-w, w + 1):
        lo, hi = max(0, -off), min(n, n - off)
        a = np.array([M[r, r + off] for r in range(lo, hi)], dtype=LD)
        if not np.any(a): continue
        for x in parts:
            p, pe = _two_prod(-a[:, None], x[lo + off:hi + off])
            s[lo:hi], se = _two_sum(s[lo:hi], p)
            e[lo:hi] += se + pe
    return s + e


def solve(A, b, transpose=False, lu=None, tol=1e-15):
    """x with A x = b (or A^T x = b): LU, two steps of iterative refinement.  The residual of the unevaluated sum x + dx of the last iterate and its correction,
    taken in twice the working precision, is asserted <= tol max|b|: the reference proves itself.  Returned: x + dx rounded to long double (one more rounding of
    2^-64 relative per entry), the proven residual relative to max|b|, the factorisation."""
    lu = lu or BandLU(A)
    sol = lu.solve_T if transpose else lu.solve
    x = sol(b)
    x = x + sol(residual2(A, (x,), b, transpose))
    dx = sol(residual2(A, (x,), b, transpose))
    res = float(np.abs(residual2(A, (x, dx), b, transpose)).max() / np.abs(b).max())
    assert res <= tol, f"the exact solve's own residual: {res:.2e} of max|b|"
    return x + dx, res, lu


# ---- energy ----
def jerk_energy(T, c):
    """J, dJ/dc (6N x 3), dJ/dT (explicit part: |jerk_i(T_i)|^2)."""
    T = np.asarray(T, dtype=LD); N = len(T)
    J = LD(0); gc = np.zeros_like(c); gT = np.zeros(N, dtype=LD)
    for i in range(N):
        ci = c[6 * i:6 * i + 6]
        for j in range(3, 6):
            for k in range(3, 6):
                w = LD(_falling(j, 3) * _falling(k, 3)) * T[i] ** (j + k - 5) / (j + k - 5)
                J += w * (ci[j] @ ci[k])
                gc[6 * i + j] += 2 * w * ci[k]
        jerk = _poly_row(T[i], 3) @ ci
        gT[i] = jerk @ jerk
    return J, gc, gT


# The jerk energy alone leaves the adjoint's linear solve without an input: the spline MINIMISES J over the knot derivatives, so dJ/dc has no component along them and
# lambda = A^-T dJ/dc needs no digit of the knot system's inverse (dropping knot_adjoint_piece's duration term from frx_minco.hpp moves such a gradient by 1e-8 at
# most).  A second objective therefore adds the reference's speed term, the one penalty that is a polynomial in (T, c) and can be restated exactly.
SPEED_PENALTY = dict(vel_max=1.0, chi=1.0)           # far below every case's speeds: active at nearly every sample; of the jerk energy's order at weight 1


def speed_penalty_overrides():
    """The settings under which the library's penalty is this term alone."""
    return dict(vel_max=SPEED_PENALTY["vel_max"], penalty_pvtb=(0.0, SPEED_PENALTY["chi"], 0.0, 0.0))


def speed_penalty(T, c, kappa, vel_max, chi):
    """P = chi sum_i sum_j omega_j (T_i / kappa) max(|v_i(s_j)|^2 - vel_max^2, 0)^3, s_j = j T_i / kappa, omega = 1/2 at j = 0 and kappa, 1 between (the speed term of the
    reference's addTimeIntPenalty at the device's abscissae), with dP/dc (6N x 3) and dP/dT."""
    T = np.asarray(T, dtype=LD); N = len(T)
    P = LD(0); gc = np.zeros_like(c); gT = np.zeros(N, dtype=LD)
    om = np.ones(kappa + 1, dtype=LD); om[0] = om[-1] = LD(0.5)
    al = np.arange(kappa + 1, dtype=LD) / kappa
    k = np.arange(6)
    for i in range(N):
        ci = c[6 * i:6 * i + 6]; step = T[i] / kappa; s = step * np.arange(kappa + 1, dtype=LD)
        b1 = np.where(k >= 1, k * s[:, None] ** np.maximum(k - 1, 0), 0)                     # (kappa + 1) x 6
        b2 = np.where(k >= 2, k * (k - 1) * s[:, None] ** np.maximum(k - 2, 0), 0)
        v = b1 @ ci; a = b2 @ ci
        viol = np.maximum((v * v).sum(axis=1) - LD(vel_max) ** 2, 0)
        P += chi * step * (om * viol ** 3).sum()
        gc[6 * i:6 * i + 6] += chi * step * b1.T @ ((om * 3 * viol ** 2 * 2)[:, None] * v)
        gT[i] = chi * (om * (3 * viol ** 2 * 2 * al * (v * a).sum(axis=1) * step + viol ** 3 / kappa)).sum()
    return P, gc, gT


class ExactCore:
    """The map (T, q) -> c, the energy F = J (+ the speed penalty: pen = dict(kappa, vel_max, chi)) and its gradient (gT, gq) at durations and waypoints taken as exact."""

    def __init__(self, T, q, head, tail, with_gradient=True, pen=None, forward_of=None):
        self.T = np.asarray(T, dtype=LD); N = len(self.T)
        self.q = np.asarray(q, dtype=LD).reshape(N - 1, 3)
        if forward_of is not None:                     # the same state under another objective: its forward solve serves
            assert np.array_equal(forward_of.T, self.T) and np.array_equal(forward_of.q, self.q)
            self.A, self.b, self.C, self.residual, self.lu = forward_of.A, forward_of.b, forward_of.C, forward_of.residual, forward_of.lu
        else:
            self.A = dense_A(self.T); self.b = rhs_b(self.q, head, tail)
            self.C, self.residual, self.lu = solve(self.A, self.b)
        lu = self.lu
        self.J, self.gc, gT = jerk_energy(self.T, self.C)
        if pen:
            P, pgc, pgT = speed_penalty(self.T, self.C, **pen)
            self.J = self.J + P; self.gc = self.gc + pgc; gT = gT + pgT
        self.pos_scale = float(np.abs(self.b).max())
        if not with_gradient: return
        self.lam, self.residual_adj, _ = solve(self.A, self.gc, transpose=True, lu=lu)
        for i, (rows, dAc) in enumerate(dA_dT_times_c(self.T, self.C)):
            gT[i] -= (self.lam[rows] * dAc).sum()
        self.gT = gT
        self.gq = self.lam[5:6 * (N - 1):6].copy() if N > 1 else np.zeros((0, 3), dtype=LD)


class Exact(ExactCore):
    """Everything about one state (tau, xi) of one candidate in one layer: f = J (+ the speed penalty) + rho sum T (no rho term in the fixed-time layers), g_tau, g_xi."""

    def __init__(self, cand, layer, tau, xi, rho=0.0, total_t=None, with_gradient=True, pen=None, forward_of=None):
        self.layer = layer; self.tau = np.asarray(tau, dtype=np.float64); self.xi = np.asarray(xi, dtype=np.float64)
        verts = waypoint_vertices(cand)
        T = forward_T(self.tau, layer, total_t)
        assert len(T) == cand.coarse_n
        ExactCore.__init__(self, T, forward_P(self.xi, verts), cand.ini_state, cand.fin_state, with_gradient, pen, forward_of)
        rho = LD(rho) if layer == "soft_c2" else LD(0)
        self.f = self.J + rho * self.T.sum()
        if not with_gradient: return
        self.g_tau = layer_T_grad(self.tau, self.gT + rho, layer, total_t)
        self.g_xi = layer_P_grad(self.xi, self.gq, verts)


def objective(cand, layer, tau, xi, rho=0.0, total_t=None, pen=None):
    return Exact(cand, layer, tau, xi, rho, total_t, with_gradient=False, pen=pen).f


# ---- metrics ----
def rel(a, b):
    a = np.asarray(a, dtype=LD); b = np.asarray(b, dtype=LD)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), LD(1e-300))) if b.size else 0.0


def coeff_err_normalised(Cdev, Cref, T):
    """test_gpu_parity.coeff_err_normalised, evaluated in long double: (worst |dc_k| h^k relative to the candidate's largest normalised coefficient, worst error of a
    piece relative to that piece's largest normalised coefficient beyond the constant term)."""
    T = np.asarray(T, dtype=LD); N = len(T)
    hk = (np.repeat(T, 6) ** np.tile(np.arange(6), N))[:, None]
    en = (np.abs(np.asarray(Cdev, dtype=LD) - np.asarray(Cref, dtype=LD)) * hk).reshape(N, 6, 3); cn = (np.abs(np.asarray(Cref, dtype=LD)) * hk).reshape(N, 6, 3)
    return float(en.max() / cn.max()), float((en.max(axis=(1, 2)) / np.maximum(cn[:, 1:, :].max(axis=(1, 2)), LD(1e-300))).max())


def block_err(g, g_exact):
    """max|g - g_exact| / max|g_exact| of ONE block (tau or xi) of a gradient: no block hides behind the other, and no |f| floor."""
    return rel(g, g_exact)
