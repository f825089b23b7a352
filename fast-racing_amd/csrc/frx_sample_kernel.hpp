// Batched sampling of trajectories (frx_trajectory_sample, include/frx.h): for every candidate of a batch and every sample time, the flat state
// p, v, a, j of the fine piece that holds the time and its SE(3) outputs (the flatness map of CPU.hpp:260-299): thrust |h| with h = a + g e3,
// the attitude R = [xB yB zB](h) as a unit quaternion (w, x, y, z), the body rates.  One row of FRX_SAMPLE_FIELDS (20) doubles per sample.
//
// Shape: one workgroup per (candidate, chunk of passes x 256 consecutive samples).  The workgroup stages the candidate's durations in LDS and
// turns them into prefix sums there (one lane, left to right: the order the header fixes).  Per pass every lane takes one sample, finds its
// piece by binary search over the prefix sums, reads the piece's 18 coefficients (the lanes of a wave share one or a few pieces: the vector L1
// serves them) and writes its row into its wave's LDS tile; the wave then stores the tile as 16-byte pieces, so that every store instruction
// covers 1 KiB of consecutive output.  The kernel only writes: it is bound by the store rate.  No atomics, no traffic between workgroups and
// no workgroup barrier after the prefix sums: a row depends on its candidate's T, C and its time alone.
#pragma once
#include <hip/hip_runtime.h>

#include "frx_math.hpp"

namespace frx {

enum { SAMPLE_THREADS = 256, SAMPLE_ROW = 20 };        // workgroup size; doubles per row (FRX_SAMPLE_FIELDS)

// dynamic LDS of a workgroup: four wave tiles of 64 rows, then the prefix sums of up to maxN pieces
__host__ __device__ inline size_t sample_lds_bytes(int maxN) { return sizeof(double) * ((size_t)SAMPLE_THREADS * SAMPLE_ROW + maxN + 1); }

// Orders this wave's LDS writes before its reads of other lanes' rows (and those reads before the next pass's writes).  A wave's LDS accesses
// are served in order, so a wavefront-scope fence costs no wait; it and the barrier stop the compiler from moving accesses across.
__device__ __forceinline__ void sample_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// times: [B][S] or null; then t_s = t0 + s dt (dt > 0) or s (total / (S - 1)) (dt == 0).  chunks: workgroups per candidate.
__global__ void __launch_bounds__(SAMPLE_THREADS) k_traj_sample(const int *__restrict__ poff, double gAcc, const double *__restrict__ T,
                                                                const double *__restrict__ C, int S, double t0, double dt,
                                                                const double *__restrict__ times, double *__restrict__ out, int chunks, int passes) {
    extern __shared__ __attribute__((aligned(16))) double smp_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double *tile = smp_lds + wave * 64 * SAMPLE_ROW;                          // this wave's [64][20] rows
    double *cum = smp_lds + SAMPLE_THREADS * SAMPLE_ROW;                      // [N + 1] prefix sums of the candidate's durations
    const int b = blockIdx.x / chunks, chunk = blockIdx.x - b * chunks;
    const int p0 = poff[b], N = poff[b + 1] - p0;
    for (int i = threadIdx.x; i < N; i += SAMPLE_THREADS) cum[i + 1] = T[p0 + i];
    __syncthreads();
    if (threadIdx.x == 0) {
        double acc = 0.0;
        cum[0] = 0.0;
        for (int i = 1; i <= N; i++) { acc = acc + cum[i]; cum[i] = acc; }
    }
    __syncthreads();
    const double total = cum[N];
    const double step = total / (double)(S - 1);                             // (used when times == null and dt == 0, where S >= 2)
    const size_t cand_row = (size_t)b * S;

    for (int pass = 0; pass < passes; pass++) {
        const long long s0 = ((long long)chunk * passes + pass) * SAMPLE_THREADS + wave * 64;   // first sample of this wave's tile
        if (s0 >= S) break;                                                  // (wave-uniform: no workgroup barrier below)
        const long long s = s0 + lane;
        if (s < S) {
            // sample time, without contraction: t0 + s dt and s step round as written (the restatement's arithmetic)
            double t = times ? times[cand_row + s] : dt > 0.0 ? __dadd_rn(t0, __dmul_rn((double)s, dt)) : __dmul_rn((double)s, step);
            t = t < 0.0 ? 0.0 : t;                                           // clamp to [0, cum[N]]; NaN stays NaN
            t = t > total ? total : t;
            int lo = 0, hi = N - 1;                                          // first piece i with t <= cum[i + 1] (NaN: the last one)
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (t <= cum[mid + 1]) hi = mid; else lo = mid + 1;
            }
            const double sl = t - cum[lo];
            const double *c = C + (size_t)(p0 + lo) * 18;
            double pos[3], vel[3], acc[3], jer[3];
            poly_eval<0>(c, sl, pos);
            poly_eval<1>(c, sl, vel);
            poly_eval<2>(c, sl, acc);
            poly_eval<3>(c, sl, jer);
            const FlatFrame fr = flat_frame(acc, gAcc);                      // frame (CPU.hpp:266-276): the check's
            const double *xB = fr.xB, *zB = fr.zB, yB1 = fr.yB1, yB2 = fr.yB2, F2 = fr.F2, invF = fr.invF, invM = fr.invM;
            // quaternion of R = [xB yB zB] (R01 = yB.x = 0): branch on the largest of (trace, R00, R11, R22), the earlier on a tie; then w >= 0
            const double R00 = xB[0], R11 = yB1, R22 = zB[2], R01 = 0.0, R02 = zB[0], R10 = xB[1], R12 = zB[1], R20 = xB[2], R21 = yB2;
            const double tr = R00 + R11 + R22;
            const bool k0 = tr >= R00 && tr >= R11 && tr >= R22, k1 = !k0 && R00 >= R11 && R00 >= R22, k2 = !k0 && !k1 && R11 >= R22;
            const double rad = k0 ? 1.0 + tr : k1 ? 1.0 + R00 - R11 - R22 : k2 ? 1.0 + R11 - R00 - R22 : 1.0 + R22 - R00 - R11;
            const double rq = sqrt(rad), fq = 0.5 / rq, hr = 0.5 * rq;                 // hr: the pivot component, fq = 1 / (4 hr)
            const double dxw = (R21 - R12) * fq, dyw = (R02 - R20) * fq, dzw = (R10 - R01) * fq;      // 4 w x, 4 w y, 4 w z over 4 pivot
            const double dxy = (R01 + R10) * fq, dxz = (R02 + R20) * fq, dyz = (R12 + R21) * fq;      // 4 x y, 4 x z, 4 y z over 4 pivot
            double qw = k0 ? hr : k1 ? dxw : k2 ? dyw : dzw;
            double qx = k0 ? dxw : k1 ? hr : k2 ? dxy : dxz;
            double qy = k0 ? dyw : k1 ? dxy : k2 ? hr : dyz;
            double qz = k0 ? dzw : k1 ? dxz : k2 ? dyz : hr;
            if (qw < 0.0) { qw = -qw; qx = -qx; qy = -qy; qz = -qz; }
            // body rates: omega_xy = (-yB.j, xB.j) / |h|; omega_z = -(xB.y dzB.z - xB.z dzB.y) / |(0, zB.z, -zB.y)|, dzB = (j - zB (zB.j)) / |h|
            const double zj = dot3(zB, jer);
            const double dz1 = (jer[1] - zB[1] * zj) * invF, dz2 = (jer[2] - zB[2] * zj) * invF;
            double *mine = tile + lane * SAMPLE_ROW;
            const double row[SAMPLE_ROW] = {pos[0], pos[1], pos[2], vel[0], vel[1], vel[2], acc[0], acc[1], acc[2], jer[0], jer[1], jer[2],
                                            sqrt(F2), qw, qx, qy, qz,
                                            -(yB1 * jer[1] + yB2 * jer[2]) * invF, dot3(xB, jer) * invF, -(xB[1] * dz2 - xB[2] * dz1) * invM};
#pragma unroll
            for (int f = 0; f < SAMPLE_ROW; f += 2) *(double2 *)(mine + f) = make_double2(row[f], row[f + 1]);
        }
        sample_wave_sync();
        // the tile's rows are consecutive in `out`: 16-byte pieces q = lane + 64 k, a store instruction writes 1 KiB of consecutive bytes
        const double2 *src = (const double2 *)tile;
        double2 v[SAMPLE_ROW / 2];
#pragma unroll
        for (int k = 0; k < SAMPLE_ROW / 2; k++) v[k] = src[lane + 64 * k];       // (rows past S: read, never stored)
        double2 *dst = (double2 *)(out + (cand_row + s0) * SAMPLE_ROW);
        if (s0 + 64 <= S) {
#pragma unroll
            for (int k = 0; k < SAMPLE_ROW / 2; k++) dst[lane + 64 * k] = v[k];
        } else {
            const int pieces = (int)(S - s0) * (SAMPLE_ROW / 2);
#pragma unroll
            for (int k = 0; k < SAMPLE_ROW / 2; k++)
                if (lane + 64 * k < pieces) dst[lane + 64 * k] = v[k];
        }
        sample_wave_sync();
    }
}

} // namespace frx
