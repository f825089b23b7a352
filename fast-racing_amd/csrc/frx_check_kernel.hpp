// Dense feasibility certificate of a batch of trajectories (frx_trajectory_check, include/frx.h): per fine piece, M + 1 samples
// s_j = j (T / M) of the flatness map of CPU.hpp:260-299 - attitude from h = a + g e3, thrust |h|, body rate |omega_xy| =
// |(xB.j, yB.j)| / |h| - and the ellipsoid's reach past every half-space of the piece's corridor, n.(p - p_k) + |E R^T n|
// (CPU.hpp:322-328) WITHOUT safeMargin, reduced to eight doubles per piece:
//   0 max reach past a face   1 max |v|   2 min |h|   3 max |h|   4 max |omega_xy|   5 max |a|
//   6 local time of the worst reach (lowest j on ties)   7 index k of its half-space (lowest k on ties)
// NaN propagates through every max / min (a sample that is not a number makes its field NaN), and every reduction is order-free,
// so a piece's row depends on nothing but its own T, coefficients and corridor.
//
// Shape: one wave per piece, its lanes striding over the samples; when M + 1 <= 32 a wave holds ppw = 64 / lpp pieces in aligned groups of
// lpp (a power of two) lanes.  A wave stages its pieces' coefficients, durations and corridor blocks in its own slice of LDS (they are the same
// for every lane of a group), each lane keeps its own running max / min, and the group reduces with __shfl_xor at the end.  No atomics, no
// traffic between workgroups.
#pragma once
#include <hip/hip_runtime.h>

#include "frx_device.hpp"

namespace frx {

// (value, index) of the worst reach: NaN beats any number, then the larger value, then the lower index
__device__ __forceinline__ bool chk_worse(double a, int ia, double b, int ib) {
    const bool na = a != a, nb = b != b;
    if (na || nb) return na && (!nb || ia < ib);
    return a > b || (a == b && ia < ib);
}

// LDS doubles of one wave: ppw pieces x (18 coefficients + the step T / M + corridor block of hstride doubles)
__host__ __device__ inline int check_wave_lds(int ppw, int hstride) { return ppw * (19 + hstride); }

__global__ void __launch_bounds__(256) k_traj_check(DevProblem dp, const double *__restrict__ T, const double *__restrict__ C, int M, double *__restrict__ out,
                                                    int lpp, int ppw, int hstride) {
    extern __shared__ double chk_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int gp0 = (blockIdx.x * (blockDim.x >> 6) + wave) * ppw;            // first piece of this wave
    const int np = gp0 < dp.P ? min(ppw, dp.P - gp0) : 0;                     // pieces this wave owns
    double *cS = chk_lds + (size_t)wave * check_wave_lds(ppw, hstride);       // [ppw][18] coefficients
    double *tS = cS + 18 * ppw;                                               // [ppw] steps
    double *hS = tS + ppw;                                                    // [ppw][hstride] corridor blocks
    for (int i = lane; i < 18 * np; i += 64) cS[i] = C[(size_t)gp0 * 18 + i];
    for (int i = lane; i < np; i += 64) tS[i] = T[gp0 + i] / M;               // step first, then multiplied (the penalty's abscissa form, cc.cu:152)
    for (int i = lane; i < hstride * np; i += 64) hS[i] = dp.hblk[(size_t)gp0 * hstride + i];
    __syncthreads();

    const int grp = lane / lpp, jl = lane - grp * lpp;
    const bool mine = grp < np;
    double vcor = -INFINITY, vspd = -INFINITY, vthl = INFINITY, vthh = -INFINITY, vbdr = -INFINITY, vacc = -INFINITY;
    int icor = 0x7fffffff;                                                    // j (Kmax + 1) + k of the worst reach
    const int KS = hstride / 4;
    if (mine) {
        const double *c = cS + 18 * grp, *hb = hS + (size_t)grp * hstride;
        const double step = tS[grp];
        const int K = (int)hb[3];
        const double e0 = dp.pc.ell[0], e1 = dp.pc.ell[1], e2 = dp.pc.ell[2], margin = dp.pc.safeMargin, gAcc = dp.pc.gAcc;
#pragma unroll 1
        for (int j = jl; j <= M; j += lpp) {
            const double s1 = step * j;
            double pos[3], vel[3], acc[3], jer[3];
            poly_eval<0>(c, s1, pos);
            poly_eval<1>(c, s1, vel);
            poly_eval<2>(c, s1, acc);
            poly_eval<3>(c, s1, jer);
            const FlatFrame fr = flat_frame(acc, gAcc);                       // attitude (CPU.hpp:266-276)
            const double *xB = fr.xB, *zB = fr.zB, yB1 = fr.yB1, yB2 = fr.yB2;
            // limits (CPU.hpp:281-299, 347-398)
            const double thr = sqrt(fr.F2);
            vspd = nan_max(vspd, sqrt(dot3(vel, vel)));
            vacc = nan_max(vacc, sqrt(dot3(acc, acc)));
            vthl = nan_min(vthl, thr);
            vthh = nan_max(vthh, thr);
            const double r0 = dot3(xB, jer), r1 = yB1 * jer[1] + yB2 * jer[2];
            vbdr = nan_max(vbdr, sqrt(r0 * r0 + r1 * r1) * fr.invF);
            // corridor (CPU.hpp:322-328): records {n, n.(p_k - org) - safeMargin} after the origin org = hb[0..2]
            const double pl[3] = {pos[0] - hb[0], pos[1] - hb[1], pos[2] - hb[2]};
#pragma unroll 2
            for (int k = 0; k < K; k++) {
                const double *n = hb + 4 + 4 * k;
                const double w0 = dot3(xB, n) * e0, w1 = (yB1 * n[1] + yB2 * n[2]) * e1, w2 = dot3(zB, n) * e2;
                const double sd = (dot3(n, pl) - (n[3] + margin)) + sqrt(w0 * w0 + w1 * w1 + w2 * w2);
                const int idx = j * KS + k;
                if (chk_worse(sd, idx, vcor, icor)) { vcor = sd; icor = idx; }
            }
        }
    }
    // reduction over the group's lanes (aligned power-of-two groups: xor offsets below lpp stay inside the group)
    for (int off = lpp >> 1; off > 0; off >>= 1) {
        const double oc = __shfl_xor(vcor, off), os = __shfl_xor(vspd, off), ol = __shfl_xor(vthl, off), oh = __shfl_xor(vthh, off);
        const double ob = __shfl_xor(vbdr, off), oa = __shfl_xor(vacc, off);
        const int oi = __shfl_xor(icor, off);
        if (chk_worse(oc, oi, vcor, icor)) { vcor = oc; icor = oi; }
        vspd = nan_max(vspd, os); vthl = nan_min(vthl, ol); vthh = nan_max(vthh, oh); vbdr = nan_max(vbdr, ob); vacc = nan_max(vacc, oa);
    }
    if (mine && jl == 0) {
        const int jw = icor / KS, kw = icor - jw * KS;
        double *o = out + (size_t)(gp0 + grp) * 8;
        o[0] = vcor; o[1] = vspd; o[2] = vthl; o[3] = vthh; o[4] = vbdr; o[5] = vacc;
        o[6] = tS[grp] * jw; o[7] = (double)kw;
    }
}

} // namespace frx
