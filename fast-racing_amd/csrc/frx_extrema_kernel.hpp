// Exact per-piece extrema of speed, acceleration, thrust and body rate (frx_trajectory_extrema, include/frx.h).  The flatness map of
// CPU.hpp:260-299 makes |v|^2, |a|^2 and |h|^2 = |a + g e3|^2 polynomials in t and omega_xy^2 = |h x j|^2 / |h|^4 a rational function of t, so the
// extrema of a piece are values at the roots of a known polynomial and at the piece's two ends - nothing is sampled.  In normalised time tau = t / T, as
// frx_traj_max_rates works (frx_geometry.cpp):
//   task 0  |v|        critical polynomial d/dtau |wv|^2               degree 7
//   task 1  |a|        d/dtau |wa|^2                                   degree 5
//   task 2  |h|        d/dtau Q, Q = |wh|^2 (min AND max)              degree 5
//   task 3  omega_xy   N' Q - 2 N Q', N = |wh x wj|^2 (degree 8)       degree 13
// Roots: roots_unit of frx_geometry.cpp - the sign changes of a polynomial on [0, 1], bracketed by the roots of its derivative (recursively from degree 1
// upwards) and refined by bisection down to adjacent doubles, at most 200 steps.  The host's recursion is run here from the bottom up: the degree-m level is
// the (deg - m)-th derivative, whose coefficient i is c[i] (deg - i) (deg - 1 - i) ... (m + 1 - i), multiplied in that order - the chain of
// dc[i] = c[i] * (deg - i) the recursion forms on its way down.  A derivative's leading coefficient is c[0] times positive integers and so is zero only
// where c[0] is: leading zeros are stripped once, at the top, as the host's strip finds them only there.
// Candidates: the roots in ascending order, then tau = 0, then tau = 1 (the host's order).  A maximum is replaced on strict >, a minimum on strict <, so the
// first candidate wins a tie; a value that is not a number takes the field and stays (nan_max / nan_min).  The host's early-out for a numerically constant
// magnitude is NOT taken: the ends are always candidates, a piece of constant speed reports that speed.
// Row: [P][10] - SPEED, ACC, THRUST_MIN, THRUST_MAX, BODY_RATE, then the local time tau T of each.  T not finite or <= 0, or a coefficient not finite: all
// ten NaN, decided once up front.  A row depends on its own T, C and g alone.
// Arithmetic: every operation that makes a number is a correctly rounded + - x / sqrt in one fixed order, none fused (#pragma clang fp contract(off) in every
// device function, the compiler's builtin for sqrt): tests/extrema_reference.py restates it operation by operation and the rows agree bit for bit.
// Shape: one lane per (piece, task); a workgroup is one wave of 64 consecutive pieces, blockIdx.y the task, so the degrees are compile-time and lanes diverge on
// the data alone (number of roots, bisection steps).  The vector polynomials live in registers (compile-time indices); the lists a lane indexes at run time -
// the critical polynomial, the current level's coefficients, two root lists - live in LDS as [slot][lane] (conflict-free 8-byte accesses):
// 14 + 14 + 13 + 13 slots x 512 B = 27 648 B static (ExtLayout<13>; another kernel may give ext_roots_unit a larger layout).  Every loop is bounded (degree, 200); no atomics, no barrier, no traffic between lanes.
#pragma once
#include <hip/hip_runtime.h>

namespace frx {

enum { EXT_TASKS = 4, EXT_FIELDS = 10, EXT_MAXDEG = 13,
       EXT_TOP = 0, EXT_LVL = 14, EXT_RA = 28, EXT_RB = 41, EXT_SLOTS = 54 };   // first slot of each per-lane list in LDS

// The per-lane lists of ext_roots_unit for polynomials of degree up to MAXDEG: TOP and LVL hold MAXDEG + 1 coefficients, the two root lists MAXDEG roots.
// ExtLayout<13> is the layout above (extrema, gates); k_traj_contain runs degree 16 on ExtLayout<16> (frx_contain_kernel.hpp).
template <int MAXDEG>
struct ExtLayout { enum { TOP = 0, LVL = MAXDEG + 1, RA = 2 * (MAXDEG + 1), RB = 2 * (MAXDEG + 1) + MAXDEG, SLOTS = 2 * (MAXDEG + 1) + 2 * MAXDEG, CAP = MAXDEG }; };
static_assert((int)ExtLayout<EXT_MAXDEG>::LVL == (int)EXT_LVL && (int)ExtLayout<EXT_MAXDEG>::RA == (int)EXT_RA && (int)ExtLayout<EXT_MAXDEG>::RB == (int)EXT_RB &&
              (int)ExtLayout<EXT_MAXDEG>::SLOTS == (int)EXT_SLOTS, "the default layout is the one the extrema and gates kernels were pinned on");

// polynomial in LDS, highest power first, degree deg, at x
__device__ __forceinline__ double ext_horner(const double *c, int deg, double x) {
#pragma clang fp contract(off)
    double v = c[0];
    for (int i = 1; i <= deg; i++) v = v * x + c[64 * i];
    return v;
}

// All sign-change roots on [0, 1], ascending, of the polynomial in lds[LAY::TOP ..] (highest power first, degree DEG before its leading zeros are
// stripped).  lds points at this lane's column; slot s is lds[64 s].  Returns the count; *roots is the list's first slot (LAY::RA or LAY::RB).
template <int DEG, class LAY = ExtLayout<EXT_MAXDEG>>
__device__ __forceinline__ int ext_roots_unit(double *lds, int *roots) {
#pragma clang fp contract(off)
    static_assert(DEG <= (int)LAY::CAP, "the layout holds the polynomial");
    enum { EXT_TOP = LAY::TOP, EXT_LVL = LAY::LVL, EXT_RA = LAY::RA, EXT_RB = LAY::RB };   // (the names of the default layout, for this one)
    int s0 = 0, deg = DEG;
    while (deg > 0 && lds[64 * (EXT_TOP + s0)] == 0.0) { s0++; deg--; }
    *roots = EXT_RA;
    if (deg <= 0) return 0;
    const double *top = lds + 64 * (EXT_TOP + s0);
    double *lvl = lds + 64 * EXT_LVL;
    int cur = EXT_RA, oth = EXT_RB, ncrit = 0;
    {                                                                    // degree 1: the (deg - 1)-th derivative
        double c0 = top[0], c1 = top[64];
        for (int d = deg; d >= 2; d--) { c0 = c0 * (double)d; c1 = c1 * (double)(d - 1); }
        const double r = -c1 / c0;
        if (r >= 0.0 && r <= 1.0) { lds[64 * cur] = r; ncrit = 1; }
    }
    for (int m = 2; m <= deg; m++) {
        for (int i = 0; i <= m; i++) {                                   // coefficients of the degree-m level
            double c = top[64 * i];
            for (int d = deg; d > m; d--) c = c * (double)(d - i);
            lvl[64 * i] = c;
        }
        const double *crit = lds + 64 * cur;
        double *out = lds + 64 * oth;
        int n = 0;
        for (int i = 0; i <= ncrit; i++) {                               // intervals of pts = {0, crit.., 1}
            double a = i == 0 ? 0.0 : crit[64 * (i - 1)], b = i == ncrit ? 1.0 : crit[64 * i];
            double fa = ext_horner(lvl, m, a);
            const double fb = ext_horner(lvl, m, b);
            double r;
            if (fa == 0.0) { if (n != 0 && out[64 * (n - 1)] == a) continue; r = a; }
            else if (fb == 0.0) r = b;
            else if ((fa < 0.0) == (fb < 0.0)) continue;
            else {
                for (int it = 0; it < 200 && b - a > 0.0; it++) {        // monotone on (a, b): plain bisection down to adjacent doubles
                    const double mid = 0.5 * (a + b);
                    if (mid <= a || mid >= b) break;
                    const double fm = ext_horner(lvl, m, mid);
                    if (fm == 0.0) { a = b = mid; break; }
                    if ((fm < 0.0) == (fa < 0.0)) { a = mid; fa = fm; } else b = mid;
                }
                r = 0.5 * (a + b);
            }
            if (n < (int)LAY::CAP) out[64 * n++] = r;                      // (at most one root an interval, m intervals at most: n <= m always)
        }
        ncrit = n;
        const int t = cur; cur = oth; oth = t;
    }
    *roots = cur;
    return ncrit;
}

// |w|^2 of a vector polynomial of degree DEG (w[k][d], lowest power first): sq[0 .. 2 DEG], by the host's i-outer, j-inner double loop
template <int DEG>
__device__ __forceinline__ void ext_sq_norm(const double (*w)[3], double *sq) {
#pragma clang fp contract(off)
#pragma unroll
    for (int k = 0; k <= 2 * DEG; k++) sq[k] = 0.0;
#pragma unroll
    for (int i = 0; i <= DEG; i++)
#pragma unroll
        for (int j = 0; j <= DEG; j++) sq[i + j] += w[i][0] * w[j][0] + w[i][1] * w[j][1] + w[i][2] * w[j][2];
}

// the vector polynomial at t by the host's running-power sum
template <int DEG>
__device__ __forceinline__ void ext_eval(const double (*w)[3], double t, double *v) {
#pragma clang fp contract(off)
    double tn = 1.0;
    v[0] = 0.0; v[1] = 0.0; v[2] = 0.0;
#pragma unroll
    for (int k = 0; k <= DEG; k++) { v[0] += w[k][0] * tn; v[1] += w[k][1] * tn; v[2] += w[k][2] * tn; tn *= t; }
}

// running extrema over the candidates in their order: the first candidate is taken as it is, a later one replaces on strict > (<) or when it is not a
// number, and a running value that is not a number stays
struct ExtBest {
    double v, t;
    bool any;
    __device__ __forceinline__ void max_of(double x, double tau) { if (!any || (v == v && (x > v || x != x))) { v = x; t = tau; } any = true; }
    __device__ __forceinline__ void min_of(double x, double tau) { if (!any || (v == v && (x < v || x != x))) { v = x; t = tau; } any = true; }
};

// critical polynomial: derivative of sq (degree D2, lowest power first) into the lane's TOP list, highest power first
template <int D2>
__device__ __forceinline__ void ext_store_derivative(const double *sq, double *lds) {
#pragma clang fp contract(off)
#pragma unroll
    for (int k = D2; k >= 1; k--) lds[64 * (EXT_TOP + D2 - k)] = (double)k * sq[k];
}

// tasks 0 - 2: extrema of |w(tau)|^2 over the roots of its derivative and the two ends; WANT_MIN adds the minimum from the same candidate list
template <int DEG, bool WANT_MIN>
__device__ __forceinline__ void ext_norm_task(const double (*w)[3], double *lds, ExtBest &hi, ExtBest &lo) {
#pragma clang fp contract(off)
    double sq[2 * DEG + 1];
    ext_sq_norm<DEG>(w, sq);
    ext_store_derivative<2 * DEG>(sq, lds);
    int rs = 0;
    const int nr = ext_roots_unit<2 * DEG - 1>(lds, &rs);
    hi.any = false; lo.any = false;
    for (int q = 0; q < nr + 2; q++) {
        const double tau = q < nr ? lds[64 * (rs + q)] : (q == nr ? 0.0 : 1.0);
        double v[3];
        ext_eval<DEG>(w, tau, v);
        const double val = v[0] * v[0] + v[1] * v[1] + v[2] * v[2];
        hi.max_of(val, tau); hi.any = true;
        if (WANT_MIN) { lo.min_of(val, tau); lo.any = true; }
    }
}

// task 3: omega_xy^2 h^2 = N / Q^2 with N = |wh x wj|^2, Q = |wh|^2; critical polynomial N' Q - 2 N Q'
__device__ __forceinline__ void ext_rate_task(const double (*wh)[3], double *lds, ExtBest &hi) {
#pragma clang fp contract(off)
    double wj[3][3];
#pragma unroll
    for (int k = 0; k <= 2; k++)
#pragma unroll
        for (int d = 0; d < 3; d++) wj[k][d] = (double)(k + 1) * wh[k + 1][d];
    double X[5][3];                                                      // wh x wj, degree 4: the tau^5 term is wh[3] x 3 wh[3] = 0 and is not formed
#pragma unroll
    for (int m = 0; m < 5; m++) { X[m][0] = 0.0; X[m][1] = 0.0; X[m][2] = 0.0; }
#pragma unroll
    for (int i = 0; i <= 3; i++)
#pragma unroll
        for (int k = 0; k <= 2; k++)
            if (i + k <= 4) {
                X[i + k][0] += wh[i][1] * wj[k][2] - wh[i][2] * wj[k][1];
                X[i + k][1] += wh[i][2] * wj[k][0] - wh[i][0] * wj[k][2];
                X[i + k][2] += wh[i][0] * wj[k][1] - wh[i][1] * wj[k][0];
            }
    double N[9], Q[7], Np[8], Qp[6], A[14], Bc[14];
    ext_sq_norm<4>(X, N);
    ext_sq_norm<3>(wh, Q);
#pragma unroll
    for (int k = 0; k <= 7; k++) Np[k] = (double)(k + 1) * N[k + 1];
#pragma unroll
    for (int k = 0; k <= 5; k++) Qp[k] = (double)(k + 1) * Q[k + 1];
#pragma unroll
    for (int m = 0; m < 14; m++) { A[m] = 0.0; Bc[m] = 0.0; }
#pragma unroll
    for (int i = 0; i <= 7; i++)
#pragma unroll
        for (int j = 0; j <= 6; j++) A[i + j] += Np[i] * Q[j];
#pragma unroll
    for (int i = 0; i <= 8; i++)
#pragma unroll
        for (int j = 0; j <= 5; j++) Bc[i + j] += N[i] * Qp[j];
#pragma unroll
    for (int m = 13; m >= 0; m--) lds[64 * (EXT_TOP + 13 - m)] = A[m] - 2.0 * Bc[m];
    int rs = 0;
    const int nr = ext_roots_unit<13>(lds, &rs);
    hi.any = false;
    for (int q = 0; q < nr + 2; q++) {
        const double tau = q < nr ? lds[64 * (rs + q)] : (q == nr ? 0.0 : 1.0);
        double hv[3], jv[3];
        ext_eval<3>(wh, tau, hv);
        ext_eval<2>(wj, tau, jv);
        const double x0 = hv[1] * jv[2] - hv[2] * jv[1], x1 = hv[2] * jv[0] - hv[0] * jv[2], x2 = hv[0] * jv[1] - hv[1] * jv[0];
        const double nv = x0 * x0 + x1 * x1 + x2 * x2, qv = hv[0] * hv[0] + hv[1] * hv[1] + hv[2] * hv[2];
        hi.max_of(nv / (qv * qv), tau); hi.any = true;
    }
}

#ifndef FRX_EXT_NO_KERNEL                                                // (frx_gates_kernel.hpp takes the device functions above and not the kernel)
// grid (ceil(P / 64), EXT_TASKS), 64 threads; out [P][EXT_FIELDS]
__global__ void __launch_bounds__(64) k_traj_extrema(int P, double g, const double *__restrict__ T, const double *__restrict__ C, double *__restrict__ out) {
#pragma clang fp contract(off)
    __shared__ double ext_lds[EXT_SLOTS * 64];
    const int lane = threadIdx.x, gp = blockIdx.x * 64 + lane, task = blockIdx.y;
    if (gp >= P) return;                                                 // (no barrier in this kernel)
    double *lds = ext_lds + lane, *o = out + (size_t)gp * EXT_FIELDS;
    const double h = T[gp];
    double c[6][3];
    bool ok = __builtin_isfinite(h) && h > 0.0;
#pragma unroll
    for (int k = 0; k < 6; k++)
#pragma unroll
        for (int d = 0; d < 3; d++) { c[k][d] = C[(size_t)gp * 18 + 3 * k + d]; ok = ok && __builtin_isfinite(c[k][d]); }
    const double nan = __builtin_nan("");
    ExtBest hi, lo;
    if (task == 0) {
        if (!ok) { o[0] = nan; o[5] = nan; return; }
        double wv[5][3], hp = h;
#pragma unroll
        for (int k = 0; k <= 4; k++) {
#pragma unroll
            for (int d = 0; d < 3; d++) wv[k][d] = (double)(k + 1) * c[k + 1][d] * hp;
            hp *= h;
        }
        ext_norm_task<4, false>(wv, lds, hi, lo);
        o[0] = __builtin_sqrt(hi.v) / h; o[5] = hi.t * h;
        return;
    }
    // tasks 1 - 3 start from the normalised acceleration
    double wa[4][3], hp = h * h;
#pragma unroll
    for (int k = 0; k <= 3; k++) {
#pragma unroll
        for (int d = 0; d < 3; d++) wa[k][d] = (double)((k + 2) * (k + 1)) * c[k + 2][d] * hp;
        hp *= h;
    }
    if (task == 1) {
        if (!ok) { o[1] = nan; o[6] = nan; return; }
        ext_norm_task<3, false>(wa, lds, hi, lo);
        o[1] = __builtin_sqrt(hi.v) / (h * h); o[6] = hi.t * h;
        return;
    }
    wa[0][2] = wa[0][2] + g * (h * h);                                   // wh: the thrust vector h^2 (a + g e3)
    if (task == 2) {
        if (!ok) { o[2] = nan; o[3] = nan; o[7] = nan; o[8] = nan; return; }
        ext_norm_task<3, true>(wa, lds, hi, lo);
        o[2] = __builtin_sqrt(lo.v) / (h * h); o[7] = lo.t * h;
        o[3] = __builtin_sqrt(hi.v) / (h * h); o[8] = hi.t * h;
        return;
    }
    if (!ok) { o[4] = nan; o[9] = nan; return; }
    ext_rate_task(wa, lds, hi);
    o[4] = __builtin_sqrt(hi.v) / h; o[9] = hi.t * h;
}
#endif

} // namespace frx
