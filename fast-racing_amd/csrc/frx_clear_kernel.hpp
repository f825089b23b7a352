// Clearance of a batch of trajectories against the obstacle cloud (frx_trajectory_clearance, include/frx.h): per fine piece, M + 1 samples
// s_j = j (T / M) of the body ellipsoid C = R E - R = [xB yB zB](h), h = a + g e3, the check's frame (flat_frame, frx_math.hpp) - against every
// cloud point o_i: u = o_i - p, q = (xB.u / e0)^2 + (yB.u / e1)^2 + (zB.u / e2)^2 (decomp_util's Ellipsoid::dist, squared), r = u.u, reduced to
//   0 sqrt(min q)   1 sqrt(min r)   2 local time s_j of the sample that attains min q   3 index i of the point that attains it
// under the total order (q, j, i): NaN beats any number, then the smaller q, then the lower j, then the lower i.  min r propagates NaN.  Every
// reduction is that order or a NaN-propagating min, so a piece's row depends on nothing but its own T, coefficients and the cloud - not on the
// launch decomposition.
//
// Shape: grid over (piece, cloud chunk), four waves per workgroup.  A workgroup walks its chunk in passes of CLEAR_PASS = 256 x 4 points: every
// lane keeps CLEAR_R = 4 points in registers (point b + 256 k + lane in slot k: coalesced) with a running (min q, its j) per slot, and
// walks the piece's samples tile by tile: CLEAR_TILE sample states (p and the three axes divided by e_i, 12 doubles each) are computed into LDS
// by the first lanes, then every lane reads a state as an LDS broadcast and tests its four points against it.  Samples are walked in ascending j,
// so `<` keeps the lowest j; a slot is its own point, so i needs no comparison until the slots are folded.  LDS does not grow with M.
// Each workgroup leaves one partial (q, r, j, i) in work[piece][chunk] and k_traj_clear_reduce folds the chunks of a piece with the same order and
// takes the square roots; with one chunk the first kernel writes the row itself.  No atomics.
#pragma once
#include <hip/hip_runtime.h>

#include "frx_device.hpp"

namespace frx {

static constexpr int CLEAR_THREADS = 256;                          // four waves
static constexpr int CLEAR_R = CLEAR_PASS / CLEAR_THREADS;         // points a lane keeps in registers: 4
static constexpr int CLEAR_STATE = 12;                             // doubles of a sample state: p, xB / e0, yB / e1, zB / e2

// (q, j, i) a before (q, j, i) b: NaN beats any number, then the smaller q, then the lower j, then the lower i
__device__ __forceinline__ bool clr_worse(double a, int ja, int ia, double b, int jb, int ib) {
    const bool na = a != a, nb = b != b;
    const bool first = ja < jb || (ja == jb && ia < ib);
    if (na || nb) return na && (!nb || first);
    return a < b || (a == b && first);
}

// q and r of one point against one sample state; every product is placed by hand so that each slot, pass and chunk runs the same arithmetic
__device__ __forceinline__ void clr_test(const double *__restrict__ s, double ox, double oy, double oz, double &q, double &r) {
    const double u0 = ox - s[0], u1 = oy - s[1], u2 = oz - s[2];          // the difference first
    const double d0 = __builtin_fma(s[3], u0, __builtin_fma(s[4], u1, s[5] * u2));
    const double d1 = __builtin_fma(s[6], u0, __builtin_fma(s[7], u1, s[8] * u2));
    const double d2 = __builtin_fma(s[9], u0, __builtin_fma(s[10], u1, s[11] * u2));
    q = __builtin_fma(d0, d0, __builtin_fma(d1, d1, d2 * d2));
    r = __builtin_fma(u0, u0, __builtin_fma(u1, u1, u2 * u2));
}

// work: [P][nchunks][4] partials (min q, min r, j, i); rows: [P][4], written here when nchunks == 1
__global__ void __launch_bounds__(CLEAR_THREADS) k_traj_clear(DevProblem dp, const double *__restrict__ T, const double *__restrict__ C, int M,
                                                              const double *__restrict__ obs, int n_obs, int chunk, int nchunks,
                                                              double *__restrict__ work, double *__restrict__ rows) {
    __shared__ double cS[18];
    __shared__ double stepS;
    __shared__ __attribute__((aligned(16))) double sS[CLEAR_TILE * CLEAR_STATE];
    __shared__ double redq[CLEAR_THREADS / 64], redr[CLEAR_THREADS / 64];
    __shared__ int redj[CLEAR_THREADS / 64], redi[CLEAR_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int piece = blockIdx.x / nchunks, ck = blockIdx.x - piece * nchunks;
    if (tid < 18) cS[tid] = C[(size_t)piece * 18 + tid];
    if (tid == 18) stepS = T[piece] / M;                                  // step first, then multiplied, as the check forms it
    const long long lo = (long long)ck * chunk;
    const int i0 = (int)lo, i1 = (int)(lo + chunk < (long long)n_obs ? lo + chunk : (long long)n_obs);   // this workgroup's points [i0, i1), never empty

    const double e0 = dp.pc.ell[0], e1 = dp.pc.ell[1], e2 = dp.pc.ell[2], gAcc = dp.pc.gAcc;
    double bq = INFINITY, br = INFINITY;                                  // the lane's best over its passes: identity (+inf, highest key)
    int bj = 0x7fffffff, bi = 0x7fffffff;

#pragma unroll 1
    for (int base = i0; base < i1; base += CLEAR_PASS) {
        double ox[CLEAR_R], oy[CLEAR_R], oz[CLEAR_R], qm[CLEAR_R];
        int jm[CLEAR_R];
#pragma unroll
        for (int k = 0; k < CLEAR_R; k++) {
            const int idx = base + k * CLEAR_THREADS + tid;
            const double *o = obs + 3 * (size_t)(idx < i1 ? idx : i1 - 1);   // a slot past the end holds the chunk's last point and is left out of the fold
            ox[k] = o[0]; oy[k] = o[1]; oz[k] = o[2];
            qm[k] = INFINITY; jm[k] = 0;                  // (a slot whose q is +inf at every sample keeps j = 0, the lowest)
        }
        double rm = INFINITY;
#pragma unroll 1
        for (int t0 = 0; t0 <= M; t0 += CLEAR_TILE) {
            __syncthreads();                                              // the tile's readers are done (first tile: the coefficients are staged)
            const int nt = min(CLEAR_TILE, M + 1 - t0);
            if (tid < nt) {
                const double s1 = stepS * (t0 + tid);
                double pos[3], acc[3];
                poly_eval<0>(cS, s1, pos);
                poly_eval<2>(cS, s1, acc);
                const FlatFrame fr = flat_frame(acc, gAcc);               // attitude: the check's frame
                double *s = sS + tid * CLEAR_STATE;
                s[0] = pos[0]; s[1] = pos[1]; s[2] = pos[2];
                s[3] = fr.xB[0] / e0; s[4] = fr.xB[1] / e0; s[5] = fr.xB[2] / e0;
                s[6] = (0.0 * fr.invM) / e1; s[7] = fr.yB1 / e1; s[8] = fr.yB2 / e1;
                s[9] = fr.zB[0] / e2; s[10] = fr.zB[1] / e2; s[11] = fr.zB[2] / e2;
            }
            __syncthreads();
#pragma unroll 1
            for (int jj = 0; jj < nt; jj++) {
                const double *s = sS + jj * CLEAR_STATE;                  // the same address in every lane: a broadcast
                double st[CLEAR_STATE];
#pragma unroll
                for (int v = 0; v < CLEAR_STATE; v++) st[v] = s[v];
                const int j = t0 + jj;
#pragma unroll
                for (int k = 0; k < CLEAR_R; k++) {
                    double q, r;
                    clr_test(st, ox[k], oy[k], oz[k], q, r);
                    // NaN -> -inf (max returns its other operand for a NaN): -inf is below every q >= 0, so the first NaN replaces and is kept for good.
                    // Ascending j: a smaller value replaces, an equal one does not.
                    const double qq = __builtin_fmax(q, -INFINITY);
                    jm[k] = qq < qm[k] ? j : jm[k];
                    qm[k] = __builtin_fmin(qm[k], qq);
                    rm = __builtin_fmin(rm, __builtin_fmax(r, -INFINITY));
                }
            }
        }
        // fold the slots in ascending i (slots past the end contribute nothing; their r is a copy of a real point's)
#pragma unroll
        for (int k = 0; k < CLEAR_R; k++) {
            const int idx = base + k * CLEAR_THREADS + tid;
            const double qk = qm[k] == -INFINITY ? (double)NAN : qm[k];            // (q >= 0: -inf can only stand for a NaN)
            if (idx < i1 && clr_worse(qk, jm[k], idx, bq, bj, bi)) { bq = qk; bj = jm[k]; bi = idx; }
        }
        br = nan_min(br, rm == -INFINITY ? (double)NAN : rm);
    }

    // across the wave, then across the waves through LDS
    for (int off = 32; off > 0; off >>= 1) {
        const double oq = __shfl_xor(bq, off), orr = __shfl_xor(br, off);
        const int oj = __shfl_xor(bj, off), oi = __shfl_xor(bi, off);
        if (clr_worse(oq, oj, oi, bq, bj, bi)) { bq = oq; bj = oj; bi = oi; }
        br = nan_min(br, orr);
    }
    if (lane == 0) { redq[wave] = bq; redr[wave] = br; redj[wave] = bj; redi[wave] = bi; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < CLEAR_THREADS / 64; w++) {
            if (clr_worse(redq[w], redj[w], redi[w], bq, bj, bi)) { bq = redq[w]; bj = redj[w]; bi = redi[w]; }
            br = nan_min(br, redr[w]);
        }
        if (nchunks == 1) {
            double *o = rows + (size_t)piece * 4;
            o[0] = sqrt(bq); o[1] = sqrt(br); o[2] = stepS * bj; o[3] = (double)bi;
        } else {
            double *o = work + ((size_t)piece * nchunks + ck) * 4;
            o[0] = bq; o[1] = br; o[2] = (double)bj; o[3] = (double)bi;  // (j <= 2^14, i < 2^24: exact)
        }
    }
}

// one wave per piece: its lanes stride over the piece's chunks, same order, then the square roots
__global__ void __launch_bounds__(CLEAR_THREADS) k_traj_clear_reduce(int P, const double *__restrict__ T, int M, const double *__restrict__ work, int nchunks,
                                                                     double *__restrict__ rows) {
    const int lane = threadIdx.x & 63, piece = blockIdx.x * (CLEAR_THREADS / 64) + (threadIdx.x >> 6);
    if (piece >= P) return;                                               // (whole waves leave: the shuffles below stay among live lanes)
    double bq = INFINITY, br = INFINITY;
    int bj = 0x7fffffff, bi = 0x7fffffff;
    for (int c = lane; c < nchunks; c += 64) {
        const double *w = work + ((size_t)piece * nchunks + c) * 4;
        const double q = w[0];
        const int j = (int)w[2], i = (int)w[3];
        if (clr_worse(q, j, i, bq, bj, bi)) { bq = q; bj = j; bi = i; }
        br = nan_min(br, w[1]);
    }
    for (int off = 32; off > 0; off >>= 1) {
        const double oq = __shfl_xor(bq, off), orr = __shfl_xor(br, off);
        const int oj = __shfl_xor(bj, off), oi = __shfl_xor(bi, off);
        if (clr_worse(oq, oj, oi, bq, bj, bi)) { bq = oq; bj = oj; bi = oi; }
        br = nan_min(br, orr);
    }
    if (lane == 0) {
        double *o = rows + (size_t)piece * 4;
        o[0] = sqrt(bq); o[1] = sqrt(br); o[2] = (T[piece] / M) * bj; o[3] = (double)bi;
    }
}

} // namespace frx
