// Exact gate passage certificate of a batch of trajectories (frx_trajectory_gates, include/frx.h).  A gate is a rectangle {c + s a + t b :
// |s| <= 1, |t| <= 1} with unit normal n = (a x b) / |a x b|.  Under the flatness map n.(p(t) - c) is a quintic on every piece, so the instants at which the
// body's centre is in the gate's plane are the roots of a known polynomial - nothing is sampled.  In normalised time tau = t / T, with w_k = c_k T^k as
// k_traj_extrema works (frx_extrema_kernel.hpp):
//   f(tau) = n.(w_0 - c) + sum_{k >= 1} (n.w_k) tau^k        (the difference first, every dot product summed x, y, z)
// Crossings of a piece: ext_roots_unit<5> of f, ascending - the recursion, zero tests and bisection of the extrema kernel on its [slot][lane] LDS lists.  A root
// that is exactly tau == 0 is dropped unless the piece is its candidate's first: a knot on the plane counts once, for the earlier piece.  An exact zero of f at a
// critical point is a root of that recursion: a touch counts as a crossing with normal speed 0.
// At a root: p, v, a by the running-power sums of ext_eval (v / T, a / T^2), then
//   h = a + g e3,  zB = h / sqrt(h.h),  yB = (0, zB.z, -zB.y) / sqrt(zB.z^2 + zB.y^2),  xB = yB x zB      (flat_frame with sqrt and division)
//   d = p - c,  s = eu.d,  t = ev.d,  ru = sqrt((e0 xB.eu)^2 + (e1 yB.eu)^2 + (e2 zB.eu)^2),  rv likewise with ev       (eu = a / |a|, ev = b / |b|)
//   MARGIN = min(|a| - |s| - ru, |b| - |t| - rv), NaN propagating;  the crossing passes when MARGIN >= 0
// Reported crossing: the least under one total order - class (0: MARGIN is NaN, 1: passes, 2: the others), then for class 2 the larger MARGIN, then the earlier
// (piece, root index).  The keys of two crossings differ, so the shape of the reduction cannot change which one wins.
// Row: [n_gates][10] - N_CROSS, N_PASS, MARGIN, TIME, PIECE, U, V, REACH_U, REACH_V, NORMAL_SPEED.  No crossing: 0, 0, -inf, 0, -1, 0...  A piece of the
// candidate with T not finite or <= 0 or a coefficient not finite, or a gate record that is not finite or has |a|, |b| or |a x b| zero: all ten NaN.
// Arithmetic: every operation that makes a number is a correctly rounded + - x / sqrt in one fixed order, none fused (#pragma clang fp contract(off) in every
// device function); tests/gates_reference.py restates it operation by operation and the rows agree bit for bit.
// Shape: one wave of 64 lanes per gate (blockIdx.x).  The wave finds its candidate by a binary search of gate_off and walks the candidate's pieces in strides of
// 64, one lane per piece; a lane keeps its own counts and its own least crossing across strides.  The counts are added and the least KEY is reduced over the
// lanes by an xor butterfly (the fields do not travel); the lane that owns the winning key sums cum[k] left to right and writes the row.  LDS: the root lists of
// one quintic, GATE_SLOTS x 512 B static.  Every loop is bounded (32, pieces / 64, degree, 200); no atomics, no barrier, no traffic between workgroups, and no
// lane leaves before the butterfly.
#pragma once
#include <hip/hip_runtime.h>

#define FRX_EXT_NO_KERNEL                                                // ext_roots_unit, ext_eval and the slot layout; k_traj_extrema lives in its own object
#include "frx_extrema_kernel.hpp"

namespace frx {

enum { GATE_ROW = 10, GATE_SLOTS = EXT_RB + 5,                          // the last slot ext_roots_unit<5> touches is EXT_RB + 4
       GATE_NAN = 0, GATE_PASS = 1, GATE_MISS = 2, GATE_NONE = 3 };     // classes of a crossing's key; GATE_NONE: the lane has no crossing

// the order of the reported crossing on (class, margin, index = 8 piece + root): is key 1 before key 2?
__device__ __forceinline__ bool gate_before(int c1, double m1, int i1, int c2, double m2, int i2) {
    if (c1 != c2) return c1 < c2;
    if (c1 == GATE_MISS && m1 != m2) return m1 > m2;
    return i1 < i2;
}

__device__ __forceinline__ double gate_dot(const double *a, const double *b) {
#pragma clang fp contract(off)
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2];
}

// the gate's frame from its record {c, a, b}: wu, wv, eu, ev, n; false when the record is not finite or degenerate
__device__ __forceinline__ bool gate_frame(const double *rec, double *wu, double *wv, double *eu, double *ev, double *n) {
#pragma clang fp contract(off)
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 9; i++) ok = ok && __builtin_isfinite(rec[i]);
    const double *a = rec + 3, *b = rec + 6;
    *wu = __builtin_sqrt(gate_dot(a, a));
    *wv = __builtin_sqrt(gate_dot(b, b));
    const double m[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
    const double mn = __builtin_sqrt(gate_dot(m, m));
#pragma unroll
    for (int d = 0; d < 3; d++) { eu[d] = a[d] / *wu; ev[d] = b[d] / *wv; n[d] = m[d] / mn; }
    return ok && *wu != 0.0 && *wv != 0.0 && mn != 0.0;
}

// the body ellipsoid's reach along the unit vector e under the frame (xB, yB = (0, yB1, yB2), zB)
__device__ __forceinline__ double gate_reach(const double *ell, const double *xB, double yB1, double yB2, const double *zB, const double *e) {
#pragma clang fp contract(off)
    const double p0 = ell[0] * gate_dot(xB, e), p1 = ell[1] * (yB1 * e[1] + yB2 * e[2]), p2 = ell[2] * gate_dot(zB, e);
    return __builtin_sqrt(p0 * p0 + p1 * p1 + p2 * p2);
}

struct GateEll { double e[3]; };

// grid n_gates, 64 threads; out [n_gates][GATE_ROW]
__global__ void __launch_bounds__(64) k_traj_gates(int B, const int *__restrict__ poff, double g, GateEll ell, const double *__restrict__ T,
                                                   const double *__restrict__ C, const int *__restrict__ gate_off, const double *__restrict__ gates,
                                                   double *__restrict__ out) {
#pragma clang fp contract(off)
    __shared__ double gate_lds[GATE_SLOTS * 64];
    const int lane = threadIdx.x, gate = blockIdx.x;
    double *lds = gate_lds + lane, *o = out + (size_t)gate * GATE_ROW;
    double rec[9];
#pragma unroll
    for (int i = 0; i < 9; i++) rec[i] = gates[(size_t)gate * 9 + i];
    double wu, wv, eu[3], ev[3], n[3];
    const bool gate_ok = gate_frame(rec, &wu, &wv, eu, ev, n);
    int b = 0;
    {                                                                    // the last b with gate_off[b] <= gate (candidates without gates repeat an offset)
        int hi = B;
        for (int it = 0; it < 32 && hi - b > 1; it++) {
            const int mid = b + ((hi - b) >> 1);
            if (gate_off[mid] <= gate) b = mid; else hi = mid;
        }
    }
    const int p0 = poff[b], np = poff[b + 1] - p0;

    bool bad = !gate_ok;
    int ncross = 0, npass = 0, cls = GATE_NONE, idx = 0x7fffffff;
    double key_m = 0.0, f_margin = 0.0, f_tau = 0.0, f_T = 0.0, f_s = 0.0, f_t = 0.0, f_ru = 0.0, f_rv = 0.0, f_ns = 0.0;
    for (int k = lane; k < np && gate_ok; k += 64) {
        const int gp = p0 + k;
        const double h = T[gp];
        double w[6][3];
        bool ok = __builtin_isfinite(h) && h > 0.0;
#pragma unroll
        for (int j = 0; j < 6; j++)
#pragma unroll
            for (int d = 0; d < 3; d++) { w[j][d] = C[(size_t)gp * 18 + 3 * j + d]; ok = ok && __builtin_isfinite(w[j][d]); }
        if (!ok) { bad = true; continue; }
        double hp = h;
#pragma unroll
        for (int j = 1; j <= 5; j++) {
#pragma unroll
            for (int d = 0; d < 3; d++) w[j][d] = w[j][d] * hp;
            hp *= h;
        }
        const double d0[3] = {w[0][0] - rec[0], w[0][1] - rec[1], w[0][2] - rec[2]};
        lds[64 * (EXT_TOP + 5)] = gate_dot(n, d0);
#pragma unroll
        for (int j = 1; j <= 5; j++) lds[64 * (EXT_TOP + 5 - j)] = gate_dot(n, w[j]);
        int rs = 0;
        const int nr = ext_roots_unit<5>(lds, &rs);
        if (nr == 0) continue;
        double wv1[5][3], wa[4][3];
#pragma unroll
        for (int j = 0; j <= 4; j++)
#pragma unroll
            for (int d = 0; d < 3; d++) wv1[j][d] = (double)(j + 1) * w[j + 1][d];
#pragma unroll
        for (int j = 0; j <= 3; j++)
#pragma unroll
            for (int d = 0; d < 3; d++) wa[j][d] = (double)((j + 2) * (j + 1)) * w[j + 2][d];
        for (int q = 0; q < nr; q++) {
            const double tau = lds[64 * (rs + q)];
            if (tau == 0.0 && k != 0) continue;
            double pos[3], vel[3], acc[3];
            ext_eval<5>(w, tau, pos);
            ext_eval<4>(wv1, tau, vel);
            ext_eval<3>(wa, tau, acc);
            const double hh = h * h;
#pragma unroll
            for (int d = 0; d < 3; d++) { vel[d] = vel[d] / h; acc[d] = acc[d] / hh; }
            const double th[3] = {acc[0], acc[1], acc[2] + g};
            const double tn = __builtin_sqrt(gate_dot(th, th));
            const double zB[3] = {th[0] / tn, th[1] / tn, th[2] / tn};
            const double yn = __builtin_sqrt(zB[2] * zB[2] + zB[1] * zB[1]);
            const double yB1 = zB[2] / yn, yB2 = -zB[1] / yn;
            const double xB[3] = {yB1 * zB[2] - yB2 * zB[1], yB2 * zB[0], -(yB1 * zB[0])};
            const double dc[3] = {pos[0] - rec[0], pos[1] - rec[1], pos[2] - rec[2]};
            const double s = gate_dot(eu, dc), t = gate_dot(ev, dc);
            const double ru = gate_reach(ell.e, xB, yB1, yB2, zB, eu), rv = gate_reach(ell.e, xB, yB1, yB2, zB, ev);
            const double mu = (wu - __builtin_fabs(s)) - ru, mv = (wv - __builtin_fabs(t)) - rv;
            const double margin = (mu != mu || mu <= mv) ? mu : mv;      // the smaller one; a NaN stays
            const int c = margin != margin ? GATE_NAN : (margin >= 0.0 ? GATE_PASS : GATE_MISS);
            ncross++;
            if (c == GATE_PASS) npass++;
            const int id = 8 * k + q;
            if (gate_before(c, margin, id, cls, key_m, idx)) {
                cls = c; key_m = margin; idx = id;
                f_margin = margin; f_tau = tau; f_T = h; f_s = s; f_t = t; f_ru = ru; f_rv = rv; f_ns = gate_dot(n, vel);
            }
        }
    }
    // over the wave: counts added, the least key by an xor butterfly - every lane is here
    const int own_cls = cls, own_idx = idx;
    int any_bad = bad ? 1 : 0;
    for (int off = 32; off > 0; off >>= 1) {
        ncross += __shfl_xor(ncross, off); npass += __shfl_xor(npass, off); any_bad |= __shfl_xor(any_bad, off);
        const int oc = __shfl_xor(cls, off), oi = __shfl_xor(idx, off);
        const double om = __shfl_xor(key_m, off);
        if (gate_before(oc, om, oi, cls, key_m, idx)) { cls = oc; key_m = om; idx = oi; }
    }
    if (any_bad) {
        if (lane == 0) {
            const double nan = __builtin_nan("");
#pragma unroll
            for (int f = 0; f < GATE_ROW; f++) o[f] = nan;
        }
        return;
    }
    if (cls == GATE_NONE) {
        if (lane == 0) {
            o[0] = 0.0; o[1] = 0.0; o[2] = -__builtin_inf(); o[3] = 0.0; o[4] = -1.0;
#pragma unroll
            for (int f = 5; f < GATE_ROW; f++) o[f] = 0.0;
        }
        return;
    }
    if (own_cls == GATE_NONE || own_idx != idx) return;
    const int kw = idx >> 3;
    double cum = 0.0;
    for (int i = 0; i < kw; i++) cum += T[p0 + i];                       // cum[k], the durations summed left to right as frx_trajectory_sample does
    o[0] = (double)ncross; o[1] = (double)npass; o[2] = f_margin; o[3] = cum + f_tau * f_T; o[4] = (double)kw;
    o[5] = f_s; o[6] = f_t; o[7] = f_ru; o[8] = f_rv; o[9] = f_ns;
}

} // namespace frx
