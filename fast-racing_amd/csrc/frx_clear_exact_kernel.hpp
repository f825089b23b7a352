// Exact clearance certificate of a batch of trajectories against the obstacle cloud (frx_trajectory_clearance_exact, include/frx.h).
// The body ellipsoid is E = diag(eh, eh, ev) in the body frame and [xB yB zB] is orthonormal, so with u = o - p, h = a + g e3, zB = h / |h|
//   q = ((u.u) - (zB.u)^2) / eh^2 + (zB.u)^2 / ev^2        (the dense kernel's q with e0 = e1: xB and yB drop out; not a number only where h = 0)
// In normalised time tau = t / T with w_k = c_k T^k and wh = T^2 (a + g e3) as k_traj_contain forms them, per (piece, cloud point o):
//   U_0 = o - w_0 (the difference first), U_k = -w_k          u(tau), a quintic
//   S = U.U (degree 10, ext_sq_norm)   Q = wh.wh (degree 6, ext_sq_norm)   m = U.wh (degree 8, i over U outer, j over wh inner)
//   r = S      q = (S - m^2 / Q) / eh^2 + (m^2 / Q) / ev^2
//   DIST task  critical polynomial S' (degree 9)
//   ELL task   F = ev^2 S' Q^2 - (ev^2 - eh^2) m (2 m' Q - m Q')  (degree 21): Q^2 times the numerator of d/dtau [ev^2 S + (eh^2 - ev^2) m^2 / Q].  Every
//              product of two polynomials is clx_mul (i over the first factor outer, j over the second inner, out[i + j] += a[i] b[j]), in the order
//              Q2 = Q Q, A = S' Q2, B1 = m' Q, B2 = m Q', G = 2 B1 - B2, H = m G, F = ev^2 A - (ev^2 - eh^2) H
// Both tasks: candidates = the roots from ext_roots_unit ascending, then tau = 0, then tau = 1; the VALUE at a candidate never comes from the expanded
// polynomial but from p and wh by ext_eval: u = o - p, S = u.u, m = u.wh, Qv = wh.wh, k = (m m) / Qv, q = (S - k) / eh^2 + k / ev^2, a q below 0 taken as 0
// (a NaN stays).  The minimum of a point by ExtBest::min_of.  Over the points each minimum is a total order: NaN first, then the smaller value, then the lower i.
// Row [P][6]: sqrt(min q), sqrt(min r), tau T of the first, its i, tau T of the second, its i.  T not finite or <= 0, or a coefficient not finite: six NaN.
//
// The cull (rigorous: it changes the work, never a row).  box = the box of the piece's six Bezier control points, widened by 2^-40 sum_k |w_k| per axis (the
// rounding of the control points and of ext_eval is some 2^-49 of that sum), so the computed p(tau) lies in it for every tau in [0, 1].  d2(o) = the squared
// distance from o to the box, its three squares summed in the order of u.u: every |u_d| the kernel forms at a candidate is at least the box's |d_d| (rounding
// is monotone), hence computed r >= d2, and q >= r / emax^2 mathematically, to a few ulps in the arithmetic above (the factor CLX_INFL = 1 + 2^-20 covers it).
// Upper bounds R_ub, Q_ub: minima of r and q AT CANDIDATES - over the whole cloud at tau = 0 and tau = 1 (k_traj_clear_exact_bounds, a launch of its own that
// leaves one pair per chunk; chunk-local bounds would let a far chunk keep all its points, which lie about as far as its own best), and the minima the
// workgroup's tasks have found so far.  Where a FINITE point has q = NaN at tau = 0 or tau = 1 (thrust zero at an end of the piece: every point has it
// there) the points tie for the ELL minimum at NaN and the lowest i must win, however far away: no number is an upper bound then, the chunk's pair holds
// NaN in place of its q, and Q_ub stays +inf for the whole piece - the q side of the cull is off, every point survives and runs its ELL task.  A point survives unless d2 > max(R_ub, emax^2 Q_ub) CLX_INFL; of a survivor the DIST task runs unless d2 > R_ub CLX_INFL,
// and the ELL task unless lb > emax^2 Q_ub CLX_INFL with lb its min r (d2 where the DIST task did not run).  A comparison that is not true, NaN included,
// runs; a cloud point that is not finite always runs everything.  A point left out therefore has a minimum strictly above one that is kept: it can neither
// win nor tie.  (Away from the ends a finite point sees q = NaN only where one of ITS candidates meets Q = 0 exactly: an isolated instant of zero thrust
// inside a piece is seen only through the surviving points' candidates.)
//
// Shape: grid (piece, cloud chunk), one wave per workgroup, for the bounds and again for the certificate.  There the wave sweeps its chunk 64 points at a time, ballot-compacts the survivors into an LDS queue of
// 128 entries in ascending i and runs one lane per queued point whenever 64 wait, and once at the end: no global survivor list, nothing to overflow.  Each
// workgroup leaves one partial (q, tau T, i, r, tau T, i, survivors, ELL tasks; slots 8 and 9 are the bounds' pair) in work[piece][chunk], 10 doubles; k_traj_clear_exact_reduce folds the chunks of
// a piece under the same orders and takes the roots; with one chunk the first kernel writes the row as well.  LDS: ext_roots_unit's lists on ExtLayout<21>,
// 86 slots x 512 B = 44 032 B, and the queue, 1 536 B.  No atomics, every loop bounded, the wave stays whole up to its last wave-wide operation.
// tests/clear_exact_reference.py restates the arithmetic operation by operation and the rows agree bit for bit.
#pragma once
#include <hip/hip_runtime.h>

#define FRX_EXT_NO_KERNEL                                                // ext_roots_unit, ext_eval, ext_sq_norm, ExtBest; k_traj_extrema lives in its own object
#include "frx_extrema_kernel.hpp"

namespace frx {

typedef ExtLayout<21> ClxLay;
enum { CLX_ROW = 6, CLX_PART = 10, CLX_SLOTS = ClxLay::SLOTS, CLX_QUEUE = 128, CLX_NONE = 0x7fffffff };
#define CLX_INFL 1.00000095367431640625                                  // 1 + 2^-20

struct ClxArgs {
    int P, n_obs, chunk, nchunks, cull;
    double g, eh, ev;
};

// out[i + j] += a[i] b[j], i outer, j inner; out has NA + NB + 1 entries, zeroed here
template <int NA, int NB>
__device__ __forceinline__ void clx_mul(const double *a, const double *b, double *out) {
#pragma clang fp contract(off)
#pragma unroll
    for (int k = 0; k <= NA + NB; k++) out[k] = 0.0;
#pragma unroll
    for (int i = 0; i <= NA; i++)
#pragma unroll
        for (int j = 0; j <= NB; j++) out[i + j] += a[i] * b[j];
}

// is (v1, i1) before (v2, i2)?  A value that is not a number first, then the smaller, then the lower point; CLX_NONE is after everything
__device__ __forceinline__ bool clx_before(double v1, int i1, double v2, int i2) {
    if (i1 == CLX_NONE) return false;
    if (i2 == CLX_NONE) return true;
    const bool n1 = v1 != v1, n2 = v2 != v2;
    if (n1 || n2) return n1 && (!n2 || i1 < i2);
    return v1 < v2 || (v1 == v2 && i1 < i2);
}

// what a workgroup knows of its piece
struct ClxPiece {
    double w[6][3], wh[4][3], Q[7], Q2[13], Qp[6];
    double lo[3], hi[3];
    double eh2, ev2, delta, emax2;
};

// r and q of the point o at tau, directly from p and wh
__device__ __forceinline__ void clx_value(const ClxPiece &pc, const double *o, double tau, double &r, double &q) {
#pragma clang fp contract(off)
    double pos[3], hv[3];
    ext_eval<5>(pc.w, tau, pos);
    ext_eval<3>(pc.wh, tau, hv);
    const double u[3] = {o[0] - pos[0], o[1] - pos[1], o[2] - pos[2]};
    const double S = u[0] * u[0] + u[1] * u[1] + u[2] * u[2];
    const double m = u[0] * hv[0] + u[1] * hv[1] + u[2] * hv[2];
    const double Qv = hv[0] * hv[0] + hv[1] * hv[1] + hv[2] * hv[2];
    const double k = (m * m) / Qv;
    double qq = (S - k) / pc.eh2 + k / pc.ev2;
    if (qq < 0.0) qq = 0.0;
    r = S; q = qq;
}

// squared distance from o to the piece's box, summed as u.u is
__device__ __forceinline__ double clx_box_d2(const ClxPiece &pc, const double *o) {
#pragma clang fp contract(off)
    double d[3];
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const double below = pc.lo[a] - o[a], above = o[a] - pc.hi[a];
        d[a] = below > 0.0 ? below : (above > 0.0 ? above : 0.0);
    }
    return d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
}

// the smallest number over the wave of the lanes' x (a NaN is no number; +inf when there is none)
__device__ __forceinline__ double clx_wave_min(double x) {
    double v = x == x ? x : __builtin_inf();
    for (int off = 32; off > 0; off >>= 1) {
        const double o = __shfl_xor(v, off);
        if (o < v) v = o;
    }
    return v;
}

// One point's tasks.  run_r / run_q: which of them run; min r -> (mr, tr), min q -> (mq, tq) (taus)
__device__ __forceinline__ void clx_tasks(const ClxPiece &pc, const double *o, double *lds, bool run_r, bool cull, double d2, double q_ub,
                                          bool &ran_r, bool &ran_q, double &mr, double &tr, double &mq, double &tq) {
#pragma clang fp contract(off)
    ran_r = false; ran_q = false;
    double U[6][3];
#pragma unroll
    for (int d = 0; d < 3; d++) U[0][d] = o[d] - pc.w[0][d];
#pragma unroll
    for (int k = 1; k <= 5; k++)
#pragma unroll
        for (int d = 0; d < 3; d++) U[k][d] = -pc.w[k][d];
    double S[11], Sp[10];
    ext_sq_norm<5>(U, S);
#pragma unroll
    for (int k = 0; k <= 9; k++) Sp[k] = (double)(k + 1) * S[k + 1];
    double lb = d2;
    if (run_r) {
#pragma unroll
        for (int k = 9; k >= 0; k--) lds[64 * (ClxLay::TOP + 9 - k)] = Sp[k];
        int rs = 0;
        const int nr = ext_roots_unit<9, ClxLay>(lds, &rs);
        ExtBest best;
        best.any = false;
        for (int c = 0; c < nr + 2; c++) {
            const double tau = c < nr ? lds[64 * (rs + c)] : (c == nr ? 0.0 : 1.0);
            double r, q;
            clx_value(pc, o, tau, r, q);
            best.min_of(r, tau);
        }
        mr = best.v; tr = best.t; ran_r = true; lb = best.v;
    }
    const bool finite = __builtin_isfinite(o[0]) && __builtin_isfinite(o[1]) && __builtin_isfinite(o[2]);
    if (cull && finite && lb > pc.emax2 * q_ub * CLX_INFL) return;
    {
        double m[9], mp[8], B1[14], B2[14], F[22], H[22];
#pragma unroll
        for (int k = 0; k <= 8; k++) m[k] = 0.0;
#pragma unroll
        for (int i = 0; i <= 5; i++)
#pragma unroll
            for (int j = 0; j <= 3; j++) m[i + j] += U[i][0] * pc.wh[j][0] + U[i][1] * pc.wh[j][1] + U[i][2] * pc.wh[j][2];
#pragma unroll
        for (int k = 0; k <= 7; k++) mp[k] = (double)(k + 1) * m[k + 1];
        clx_mul<9, 12>(Sp, pc.Q2, F);                                    // A
        clx_mul<7, 6>(mp, pc.Q, B1);
        clx_mul<8, 5>(m, pc.Qp, B2);
#pragma unroll
        for (int k = 0; k <= 13; k++) B1[k] = 2.0 * B1[k] - B2[k];       // G
        clx_mul<8, 13>(m, B1, H);
#pragma unroll
        for (int k = 21; k >= 0; k--) lds[64 * (ClxLay::TOP + 21 - k)] = pc.ev2 * F[k] - pc.delta * H[k];
    }
    int rs = 0;
    const int nr = ext_roots_unit<21, ClxLay>(lds, &rs);
    ExtBest best;
    best.any = false;
    for (int c = 0; c < nr + 2; c++) {
        const double tau = c < nr ? lds[64 * (rs + c)] : (c == nr ? 0.0 : 1.0);
        double r, q;
        clx_value(pc, o, tau, r, q);
        best.min_of(q, tau);
    }
    mq = best.v; tq = best.t; ran_q = true;
}

// the piece's T and coefficients -> pc; false when T is not finite or <= 0 or a coefficient is not finite (the same verdict in every lane)
__device__ __forceinline__ bool clx_setup(const ClxArgs &a, const double *__restrict__ T, const double *__restrict__ C, int piece, ClxPiece &pc, double &h) {
#pragma clang fp contract(off)
    h = T[piece];
    bool ok = __builtin_isfinite(h) && h > 0.0;
#pragma unroll
    for (int i = 0; i < 6; i++)
#pragma unroll
        for (int d = 0; d < 3; d++) { pc.w[i][d] = C[(size_t)piece * 18 + 3 * i + d]; ok = ok && __builtin_isfinite(pc.w[i][d]); }
    if (!ok) return false;
    {
        double hp = h;
#pragma unroll
        for (int i = 1; i <= 5; i++) {
#pragma unroll
            for (int d = 0; d < 3; d++) pc.w[i][d] = pc.w[i][d] * hp;
            hp *= h;
        }
#pragma unroll
        for (int i = 0; i <= 3; i++)
#pragma unroll
            for (int d = 0; d < 3; d++) pc.wh[i][d] = (double)((i + 2) * (i + 1)) * pc.w[i + 2][d];
        pc.wh[0][2] = pc.wh[0][2] + a.g * (h * h);
        ext_sq_norm<3>(pc.wh, pc.Q);
        clx_mul<6, 6>(pc.Q, pc.Q, pc.Q2);
#pragma unroll
        for (int k = 0; k <= 5; k++) pc.Qp[k] = (double)(k + 1) * pc.Q[k + 1];
        pc.eh2 = a.eh * a.eh; pc.ev2 = a.ev * a.ev; pc.delta = pc.ev2 - pc.eh2;
        pc.emax2 = pc.eh2 > pc.ev2 ? pc.eh2 : pc.ev2;
        // the box of the Bezier control points b_j = sum_{k <= j} (C(j, k) / C(5, k)) w_k, widened
        const double bez[6][6] = {{1.0, 0.0, 0.0, 0.0, 0.0, 0.0}, {1.0, 0.2, 0.0, 0.0, 0.0, 0.0}, {1.0, 0.4, 0.1, 0.0, 0.0, 0.0},
                                  {1.0, 0.6, 0.3, 0.1, 0.0, 0.0}, {1.0, 0.8, 0.6, 0.4, 0.2, 0.0}, {1.0, 1.0, 1.0, 1.0, 1.0, 1.0}};
#pragma unroll
        for (int d = 0; d < 3; d++) {
            double lo = pc.w[0][d], hi = pc.w[0][d], sum = 0.0;
#pragma unroll
            for (int j = 1; j <= 5; j++) {
                double b = pc.w[0][d];
#pragma unroll
                for (int k = 1; k <= j; k++) b += bez[j][k] * pc.w[k][d];
                lo = b < lo ? b : lo; hi = b > hi ? b : hi;
            }
#pragma unroll
            for (int k = 0; k <= 5; k++) sum += __builtin_fabs(pc.w[k][d]);
            const double pad = sum * 9.094947017729282379150390625e-13;  // 2^-40
            pc.lo[d] = lo - pad; pc.hi[d] = hi + pad;
        }
    }
    return true;
}

// grid P x nchunks, 64 threads: the least r and the least q of the chunk's points at tau = 0 and at tau = 1 (values at candidates: upper bounds of the piece's
// minima) into work[piece][chunk][8], [9]; +inf where there is no number.  A piece that is not valid gets none: nobody reads them.
__global__ void __launch_bounds__(64) k_traj_clear_exact_bounds(ClxArgs a, const double *__restrict__ T, const double *__restrict__ C,
                                                                const double *__restrict__ obs, double *__restrict__ work) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x;
    const int piece = blockIdx.x / a.nchunks, ck = blockIdx.x - piece * a.nchunks;
    ClxPiece pc;
    double h;
    if (!clx_setup(a, T, C, piece, pc, h)) return;
    const long long c0 = (long long)ck * a.chunk;
    const int i0 = (int)c0, i1 = (int)(c0 + a.chunk < (long long)a.n_obs ? c0 + a.chunk : (long long)a.n_obs);
    double rb = __builtin_inf(), qb = __builtin_inf();
    bool qnan = false;                                                   // a FINITE point has q = NaN at an end of the piece
#pragma unroll 1
    for (int idx = i0 + lane; idx < i1; idx += 64) {
        const double *op = obs + 3 * (size_t)idx;
        const double o[3] = {op[0], op[1], op[2]};
        double r0, q0, r1, q1;
        clx_value(pc, o, 0.0, r0, q0);
        clx_value(pc, o, 1.0, r1, q1);
        if (r0 < rb) rb = r0;
        if (r1 < rb) rb = r1;
        if (q0 < qb) qb = q0;
        if (q1 < qb) qb = q1;
        if ((q0 != q0 || q1 != q1) && __builtin_isfinite(o[0]) && __builtin_isfinite(o[1]) && __builtin_isfinite(o[2])) qnan = true;
    }
    rb = clx_wave_min(rb); qb = clx_wave_min(qb);                        // (every lane is here)
    if (__ballot(qnan) != 0ull) qb = __builtin_nan("");                  // no number bounds min q from above: a NaN is the least value of the order
    if (lane == 0) {
        double *part = work + ((size_t)piece * a.nchunks + ck) * CLX_PART;
        part[8] = rb; part[9] = qb;
    }
}

// grid P x nchunks, 64 threads, after k_traj_clear_exact_bounds.  work: [P][nchunks][CLX_PART]; rows: [P][CLX_ROW], written here when nchunks == 1
__global__ void __launch_bounds__(64) k_traj_clear_exact(ClxArgs a, const double *__restrict__ T, const double *__restrict__ C, const double *__restrict__ obs,
                                                         double *__restrict__ work, double *__restrict__ rows) {
#pragma clang fp contract(off)
    __shared__ double clx_lds[CLX_SLOTS * 64];
    __shared__ double qd[CLX_QUEUE];
    __shared__ int qi[CLX_QUEUE];
    const int lane = threadIdx.x;
    const int piece = blockIdx.x / a.nchunks, ck = blockIdx.x - piece * a.nchunks;
    double *lds = clx_lds + lane;
    double *part = work + ((size_t)piece * a.nchunks + ck) * CLX_PART;
    const double nan = __builtin_nan("");

    ClxPiece pc;
    double h;
    if (!clx_setup(a, T, C, piece, pc, h)) {                             // (the whole wave leaves)
        if (lane == 0) {
#pragma unroll
            for (int f = 0; f < 6; f++) part[f] = nan;
            part[6] = 0.0; part[7] = 0.0;
            if (a.nchunks == 1)
#pragma unroll
                for (int f = 0; f < CLX_ROW; f++) rows[(size_t)piece * CLX_ROW + f] = nan;
        }
        return;
    }

    const bool cull = a.cull != 0;
    const long long c0 = (long long)ck * a.chunk;
    const int i0 = (int)c0, i1 = (int)(c0 + a.chunk < (long long)a.n_obs ? c0 + a.chunk : (long long)a.n_obs);   // this workgroup's points [i0, i1), never empty
    bool qoff = false;
    double r_ub = __builtin_inf(), q_ub = __builtin_inf();               // the same in every lane: the least bound of the piece's chunks to begin with
    {
        const double *w0 = work + (size_t)piece * a.nchunks * CLX_PART;
        for (int c = lane; c < a.nchunks; c += 64) {
            const double rb = w0[(size_t)c * CLX_PART + 8], qb = w0[(size_t)c * CLX_PART + 9];
            if (rb < r_ub) r_ub = rb;
            if (qb < q_ub) q_ub = qb;
            if (qb != qb) qoff = true;
        }
        r_ub = clx_wave_min(r_ub); q_ub = clx_wave_min(q_ub);
        qoff = __ballot(qoff) != 0ull;
        if (qoff) q_ub = __builtin_inf();                                // q = NaN at an end of the piece: the q side of the cull is off for good
    }
    double bq = 0.0, btq = 0.0, br = 0.0, btr = 0.0;                     // the lane's best of each order
    int biq = CLX_NONE, bir = CLX_NONE;
    int qn = 0, nsurv = 0, nell = 0;

#pragma unroll 1
    for (int base = i0; base < i1 || qn > 0; base += 64) {
        const bool sweep = base < i1;                                    // (the last turn only empties the queue)
        if (sweep) {
            const int idx = base + lane;
            const bool have = idx < i1;
            const double *op = obs + 3 * (size_t)(have ? idx : i1 - 1);
            const double o[3] = {op[0], op[1], op[2]};
            const double d2 = clx_box_d2(pc, o);
            const double bound = pc.emax2 * q_ub, thr = (r_ub > bound ? r_ub : bound) * CLX_INFL;
            const bool finite = __builtin_isfinite(o[0]) && __builtin_isfinite(o[1]) && __builtin_isfinite(o[2]);
            const bool surv = have && !(cull && finite && d2 > thr);
            const unsigned long long mask = __ballot(surv);
            if (surv) {
                const int at = qn + __popcll(mask & ((1ull << lane) - 1ull));
                qi[at] = idx; qd[at] = d2;
            }
            const int ns = __popcll(mask);
            qn += ns; nsurv += ns;
            __syncthreads();
        }
        if (qn >= 64 || (!sweep && qn > 0)) {
            const int n = qn < 64 ? qn : 64;
            const bool mine = lane < n;
            bool ran_r = false, ran_q = false;
            if (mine) {
                const int idx = qi[lane];
                const double d2 = qd[lane];
                const double *op = obs + 3 * (size_t)idx;
                const double o[3] = {op[0], op[1], op[2]};
                const bool finite = __builtin_isfinite(o[0]) && __builtin_isfinite(o[1]) && __builtin_isfinite(o[2]);
                const bool run_r = !(cull && finite && d2 > r_ub * CLX_INFL);
                double mr = 0.0, tr = 0.0, mq = 0.0, tq = 0.0;
                clx_tasks(pc, o, lds, run_r, cull, d2, q_ub, ran_r, ran_q, mr, tr, mq, tq);
                if (ran_r && clx_before(mr, idx, br, bir)) { br = mr; btr = tr; bir = idx; }
                if (ran_q && clx_before(mq, idx, bq, biq)) { bq = mq; btq = tq; biq = idx; }
            }
            nell += __popcll(__ballot(ran_q));
            r_ub = __builtin_fmin(r_ub, clx_wave_min(bir != CLX_NONE ? br : nan));
            // (a lane whose best has become NaN - a point that is not finite - has no number to offer from then on: the bounds lose that lane's share of
            // the tightening, which costs work and never a row)
            if (!qoff) q_ub = __builtin_fmin(q_ub, clx_wave_min(biq != CLX_NONE ? bq : nan));
            __syncthreads();
            const int rest = qn - n;                                     // < 64: move the tail of the queue to its head
            int ti = 0; double td = 0.0;
            if (lane < rest) { ti = qi[64 + lane]; td = qd[64 + lane]; }
            __syncthreads();
            if (lane < rest) { qi[lane] = ti; qd[lane] = td; }
            __syncthreads();
            qn = rest;
        }
    }

    // over the wave: the least key of each order - every lane is here
    for (int off = 32; off > 0; off >>= 1) {
        const double oq = __shfl_xor(bq, off), otq = __shfl_xor(btq, off), orr = __shfl_xor(br, off), otr = __shfl_xor(btr, off);
        const int oiq = __shfl_xor(biq, off), oir = __shfl_xor(bir, off);
        if (clx_before(oq, oiq, bq, biq)) { bq = oq; btq = otq; biq = oiq; }
        if (clx_before(orr, oir, br, bir)) { br = orr; btr = otr; bir = oir; }
    }
    if (lane == 0) {
        part[0] = bq; part[1] = btq * h; part[2] = (double)biq;          // (i < 2^24: exact)
        part[3] = br; part[4] = btr * h; part[5] = (double)bir;
        part[6] = (double)nsurv; part[7] = (double)nell;
        if (a.nchunks == 1) {
            double *o = rows + (size_t)piece * CLX_ROW;
            o[0] = __builtin_sqrt(bq); o[1] = __builtin_sqrt(br); o[2] = btq * h; o[3] = (double)biq; o[4] = btr * h; o[5] = (double)bir;
        }
    }
}

// one wave per piece: its lanes stride over the piece's chunks, the same orders, then the square roots
__global__ void __launch_bounds__(64) k_traj_clear_exact_reduce(int P, int nchunks, const double *__restrict__ work, double *__restrict__ rows) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x, piece = blockIdx.x;
    double *o = rows + (size_t)piece * CLX_ROW;
    const double *w0 = work + (size_t)piece * nchunks * CLX_PART;
    if (w0[2] != w0[2]) {                                                // the piece is not valid: six NaN in every chunk (the same verdict in every lane)
        if (lane == 0)
#pragma unroll
            for (int f = 0; f < CLX_ROW; f++) o[f] = __builtin_nan("");
        return;
    }
    double bq = 0.0, btq = 0.0, br = 0.0, btr = 0.0;
    int biq = CLX_NONE, bir = CLX_NONE;
    for (int c = lane; c < nchunks; c += 64) {
        const double *w = w0 + (size_t)c * CLX_PART;
        const int iq = (int)w[2], ir = (int)w[5];
        if (clx_before(w[0], iq, bq, biq)) { bq = w[0]; btq = w[1]; biq = iq; }
        if (clx_before(w[3], ir, br, bir)) { br = w[3]; btr = w[4]; bir = ir; }
    }
    for (int off = 32; off > 0; off >>= 1) {
        const double oq = __shfl_xor(bq, off), otq = __shfl_xor(btq, off), orr = __shfl_xor(br, off), otr = __shfl_xor(btr, off);
        const int oiq = __shfl_xor(biq, off), oir = __shfl_xor(bir, off);
        if (clx_before(oq, oiq, bq, biq)) { bq = oq; btq = otq; biq = oiq; }
        if (clx_before(orr, oir, br, bir)) { br = orr; btr = otr; bir = oir; }
    }
    if (lane == 0) { o[0] = __builtin_sqrt(bq); o[1] = __builtin_sqrt(br); o[2] = btq; o[3] = (double)biq; o[4] = btr; o[5] = (double)bir; }
    (void)P;
}

} // namespace frx
