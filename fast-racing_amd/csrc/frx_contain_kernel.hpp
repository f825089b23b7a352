// Exact corridor containment certificate of a batch of trajectories (frx_trajectory_contain, include/frx.h).  The body ellipsoid is
// E = diag(eh, eh, ev) in the body frame, the face normals are unit vectors and [xB yB zB] is orthonormal, so the reach past a face is
//   |E R^T n|^2 = eh^2 + Delta (zB.n)^2,   Delta = ev^2 - eh^2,   zB = h / |h|,   h = a + g e3
// and with d = n.(p - p_k) + slack (quintic), Q = h.h (degree 6), u = n.h (cubic) the body touches the face exactly where
//   F = (d^2 - eh^2) Q - Delta u^2 = 0   and   d <= 0                                            (degree 16)
// (roots of F with d > 0 belong to the far side of the ellipsoid).  Between two consecutive contact instants sd = d + reach keeps its sign: nothing is sampled.
// In normalised time tau = t / T with w_k = c_k T^k as k_traj_gates works, wh = T^2 (a + g e3) as k_traj_extrema's thrust vector (Q and u^2 both carry
// T^4, the roots of F do not move).  Per (piece, face k), with the face's record {n, c} of the handle's hblk block (origin org, c = n.(p_k - org) - margin):
//   d_0 = (n.(w_0 - org) - (c + margin)) + slack,  d_i = n.w_i      (the constant as k_traj_check forms its distance, every dot product summed x, y, z)
//   quartic task   roots of d' by ext_roots_unit<4>; candidates: the roots ascending, tau = 0, tau = 1; d by Horner; the maximum with the rules of ExtBest
//   skip           max d + max(eh, ev) < 0: the body cannot reach the face, no contact
//   degree 16      D2 = d d (i outer, j inner), A = D2 with A_0 - eh eh, Q = |wh|^2 (ext_sq_norm), u_i = n.wh_i, U2 = u u, F = A Q (i outer, j inner), then
//                  F_m - Delta U2_m for m <= 6; roots by ext_roots_unit<16>; a root is a CONTACT when d(root) <= 0 (Horner); an exact root tau == 0 is
//                  dropped unless the piece is its candidate's first (a knot on a contact counts once, for the earlier piece)
//   intervals      of {0, contacts.., 1} with b > a, classed at the midpoint 0.5 (a + b) by the direct formula sd = ((n.(p - org) - (c + margin)) + slack) +
//                  sqrt(eh eh + Delta ((u u) / Q)) with p, wh by the running-power sums of ext_eval; !(sd <= 0) is outside.  The face's outside time is the
//                  left-to-right sum of (b - a) over its outside intervals, times T; its first excursion is its first run of outside intervals
// Piece row [P][8]: N_CONTACT (sum over faces), OUTSIDE (max over faces), T_EXIT / T_ENTER / K_EXIT of the earliest excursion (lowest k on a tie; -1 -1 -1 when
// there is none), CENTRE / T_CENTRE / K_CENTRE the largest max d (a value that is not a number first, then the larger, then the lower k).  T not finite or <= 0,
// or a coefficient not finite: all eight NaN, decided once up front.  A row depends on its piece's own T, C, faces, g, eh, ev, slack and on whether the piece
// is its candidate's first - on nothing else in the batch.
// Arithmetic: every operation that makes a number is a correctly rounded + - x / sqrt in one fixed order, none fused (#pragma clang fp contract(off) in every
// device function); tests/contain_reference.py restates it operation by operation and the rows agree bit for bit.
// Shape: one lane per (piece, face).  The faces of a piece take an aligned group of G lanes, G the smallest power of two >= Kmax and at most 64, 64 / G pieces
// per one-wave workgroup; faces beyond G by a stride loop in ascending k.  The group reduces with an xor butterfly of offsets below G: a sum of integers, a
// maximum of numbers and two total orders whose keys differ between faces, so the packing cannot change a row; the lane that owns a winning key writes its
// fields.  LDS: the per-lane lists of ext_roots_unit on ExtLayout<16>, 66 slots x 512 B = 33 792 B static.  Every loop is bounded (32, K / G, degree, 200); no
// barrier, no atomics, no traffic between workgroups, and no lane leaves before the butterfly.
#pragma once
#include <hip/hip_runtime.h>

#define FRX_EXT_NO_KERNEL                                                // ext_roots_unit, ext_eval, ext_sq_norm, ExtBest; k_traj_extrema lives in its own object
#include "frx_extrema_kernel.hpp"

namespace frx {

typedef ExtLayout<16> ConLay;
enum { CON_ROW = 8, CON_SLOTS = ConLay::SLOTS, CON_NONE = 0x7fffffff };  // CON_NONE: the face index of "no excursion / no face yet"

struct ConArgs {
    int P, B, Kmax, lg;                                                  // lg = log2 G
    double g, eh, ev, margin, slack;
    const int *poff;                                                     // [B + 1]
    const double *hblk;                                                  // [P][Kmax + 1][4], frx_device.hpp
};

__device__ __forceinline__ double con_dot(const double *a, const double *b) {
#pragma clang fp contract(off)
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2];
}

// d (lowest power first) at x by Horner
__device__ __forceinline__ double con_d_at(const double *d, double x) {
#pragma clang fp contract(off)
    double v = d[5];
#pragma unroll
    for (int i = 4; i >= 0; i--) v = v * x + d[i];
    return v;
}

// is the excursion (t1, k1) before (t2, k2)?  The earlier start, then the lower face; CON_NONE is after everything
__device__ __forceinline__ bool con_exit_before(double t1, int k1, double t2, int k2) {
    if (k1 == CON_NONE) return false;
    if (k2 == CON_NONE) return true;
    return t1 < t2 || (t1 == t2 && k1 < k2);
}

// is the centre (v1, k1) before (v2, k2)?  A value that is not a number first, then the larger, then the lower face; CON_NONE is after everything
__device__ __forceinline__ bool con_centre_before(double v1, int k1, double v2, int k2) {
    if (k1 == CON_NONE) return false;
    if (k2 == CON_NONE) return true;
    const bool n1 = v1 != v1, n2 = v2 != v2;
    if (n1 || n2) return n1 && (!n2 || k1 < k2);
    return v1 > v2 || (v1 == v2 && k1 < k2);
}

// grid ceil(P / (64 >> lg)), 64 threads; out [P][CON_ROW]
__global__ void __launch_bounds__(64) k_traj_contain(ConArgs a, const double *__restrict__ T, const double *__restrict__ C, double *__restrict__ out) {
#pragma clang fp contract(off)
    __shared__ double con_lds[CON_SLOTS * 64];
    const int lane = threadIdx.x, G = 1 << a.lg, grp = lane >> a.lg, j = lane & (G - 1);
    const int gp = blockIdx.x * (64 >> a.lg) + grp;
    const bool mine = gp < a.P;
    double *lds = con_lds + lane;

    int ncon = 0, ex_k = CON_NONE, ce_k = CON_NONE;
    double outside = 0.0, ex_t = 0.0, ex_e = 0.0, ce_v = 0.0, ce_t = 0.0;
    bool ok = false;
    if (mine) {
        const double h = T[gp];
        double w[6][3];
        ok = __builtin_isfinite(h) && h > 0.0;
#pragma unroll
        for (int i = 0; i < 6; i++)
#pragma unroll
            for (int d = 0; d < 3; d++) { w[i][d] = C[(size_t)gp * 18 + 3 * i + d]; ok = ok && __builtin_isfinite(w[i][d]); }
        if (ok) {
            int b = 0;
            {                                                            // the last b with poff[b] <= gp: is this piece its candidate's first?
                int hi = a.B;
                for (int it = 0; it < 32 && hi - b > 1; it++) {
                    const int mid = b + ((hi - b) >> 1);
                    if (a.poff[mid] <= gp) b = mid; else hi = mid;
                }
            }
            const bool first = a.poff[b] == gp;
            const double *hb = a.hblk + (size_t)gp * (size_t)(4 * (a.Kmax + 1));
            const double org[3] = {hb[0], hb[1], hb[2]};
            int K = (int)hb[3];
            if (K > a.Kmax) K = a.Kmax;
            double hp = h;
#pragma unroll
            for (int i = 1; i <= 5; i++) {
#pragma unroll
                for (int d = 0; d < 3; d++) w[i][d] = w[i][d] * hp;
                hp *= h;
            }
            double wh[4][3], Q[7];
#pragma unroll
            for (int i = 0; i <= 3; i++)
#pragma unroll
                for (int d = 0; d < 3; d++) wh[i][d] = (double)((i + 2) * (i + 1)) * w[i + 2][d];
            wh[0][2] = wh[0][2] + a.g * (h * h);
            ext_sq_norm<3>(wh, Q);
            const double eh2 = a.eh * a.eh, delta = a.ev * a.ev - eh2, emax = a.eh > a.ev ? a.eh : a.ev;
            const double d0[3] = {w[0][0] - org[0], w[0][1] - org[1], w[0][2] - org[2]};
            for (int k = j; k < K; k += G) {
                const double *rec = hb + 4 + 4 * k;
                const double n[3] = {rec[0], rec[1], rec[2]}, cm = rec[3] + a.margin;
                double d[6];
                d[0] = (con_dot(n, d0) - cm) + a.slack;
#pragma unroll
                for (int i = 1; i <= 5; i++) d[i] = con_dot(n, w[i]);
                // the quartic task: max d over the roots of d' and the two ends
#pragma unroll
                for (int i = 0; i <= 4; i++) lds[64 * (ConLay::TOP + 4 - i)] = (double)(i + 1) * d[i + 1];
                int rs = 0;
                int nr = ext_roots_unit<4, ConLay>(lds, &rs);
                ExtBest best;
                best.any = false;
                for (int q = 0; q < nr + 2; q++) {
                    const double tau = q < nr ? lds[64 * (rs + q)] : (q == nr ? 0.0 : 1.0);
                    best.max_of(con_d_at(d, tau), tau);
                }
                if (con_centre_before(best.v, k, ce_v, ce_k)) { ce_v = best.v; ce_t = best.t * h; ce_k = k; }
                if (best.v + emax < 0.0) continue;                       // the body cannot reach this face
                // the degree-16 task
                {
                    double A[11], u[4], U2[7], F[17];
#pragma unroll
                    for (int m = 0; m < 11; m++) A[m] = 0.0;
#pragma unroll
                    for (int i = 0; i <= 5; i++)
#pragma unroll
                        for (int i2 = 0; i2 <= 5; i2++) A[i + i2] += d[i] * d[i2];
                    A[0] = A[0] - eh2;
#pragma unroll
                    for (int i = 0; i <= 3; i++) u[i] = con_dot(n, wh[i]);
#pragma unroll
                    for (int m = 0; m < 7; m++) U2[m] = 0.0;
#pragma unroll
                    for (int i = 0; i <= 3; i++)
#pragma unroll
                        for (int i2 = 0; i2 <= 3; i2++) U2[i + i2] += u[i] * u[i2];
#pragma unroll
                    for (int m = 0; m < 17; m++) F[m] = 0.0;
#pragma unroll
                    for (int i = 0; i <= 10; i++)
#pragma unroll
                        for (int i2 = 0; i2 <= 6; i2++) F[i + i2] += A[i] * Q[i2];
#pragma unroll
                    for (int m = 0; m <= 6; m++) F[m] = F[m] - delta * U2[m];
#pragma unroll
                    for (int m = 0; m <= 16; m++) lds[64 * (ConLay::TOP + 16 - m)] = F[m];
                }
                nr = ext_roots_unit<16, ConLay>(lds, &rs);
                double a0 = 0.0, acc = 0.0, fe_t = 0.0, fe_e = 0.0;
                bool have = false, open = false;
                for (int q = 0; q <= nr; q++) {                          // the contacts, then the end tau = 1
                    double bb = 1.0;
                    if (q < nr) {
                        bb = lds[64 * (rs + q)];
                        if (!(con_d_at(d, bb) <= 0.0)) continue;         // the far side of the ellipsoid
                        if (bb == 0.0 && !first) continue;
                        ncon++;
                    }
                    if (bb > a0) {
                        const double mid = 0.5 * (a0 + bb);
                        double pos[3], hv[3];
                        ext_eval<5>(w, mid, pos);
                        ext_eval<3>(wh, mid, hv);
                        const double pl[3] = {pos[0] - org[0], pos[1] - org[1], pos[2] - org[2]};
                        const double dv = (con_dot(n, pl) - cm) + a.slack, qv = con_dot(hv, hv), uv = con_dot(n, hv);
                        const double sd = dv + __builtin_sqrt(eh2 + delta * ((uv * uv) / qv));
                        if (!(sd <= 0.0)) {
                            acc += bb - a0;
                            if (!have) { have = true; open = true; fe_t = a0; fe_e = bb; }
                            else if (open) fe_e = bb;
                        } else open = false;
                    }
                    a0 = bb;
                }
                const double ot = acc * h;
                if (ot > outside) outside = ot;
                if (have && con_exit_before(fe_t * h, k, ex_t, ex_k)) { ex_t = fe_t * h; ex_e = fe_e * h; ex_k = k; }
            }
        }
    }
    // over the group: the count added, the largest outside time, the least key of each order - every lane is here
    const int own_ex = ex_k, own_ce = ce_k;
    for (int off = G >> 1; off > 0; off >>= 1) {
        ncon += __shfl_xor(ncon, off);
        const double oo = __shfl_xor(outside, off), oxt = __shfl_xor(ex_t, off), ocv = __shfl_xor(ce_v, off);
        const int oxk = __shfl_xor(ex_k, off), ock = __shfl_xor(ce_k, off);
        if (oo > outside) outside = oo;
        if (con_exit_before(oxt, oxk, ex_t, ex_k)) { ex_t = oxt; ex_k = oxk; }
        if (con_centre_before(ocv, ock, ce_v, ce_k)) { ce_v = ocv; ce_k = ock; }
    }
    if (!mine) return;
    double *o = out + (size_t)gp * CON_ROW;
    if (!ok) {
        if (j == 0) {
            const double nan = __builtin_nan("");
#pragma unroll
            for (int f = 0; f < CON_ROW; f++) o[f] = nan;
        }
        return;
    }
    if (j == 0) {
        o[0] = (double)ncon; o[1] = outside;
        if (ex_k == CON_NONE) { o[2] = -1.0; o[3] = -1.0; o[4] = -1.0; }
        if (ce_k == CON_NONE) { o[5] = -__builtin_inf(); o[6] = -1.0; o[7] = -1.0; }   // (a piece without faces: no handle makes one)
    }
    if (own_ex != CON_NONE && own_ex == ex_k) { o[2] = ex_t; o[3] = ex_e; o[4] = (double)ex_k; }
    if (own_ce != CON_NONE && own_ce == ce_k) { o[5] = ce_v; o[6] = ce_t; o[7] = (double)ce_k; }
}

} // namespace frx
