// H -> V vertex enumeration on the device for a BATCH of polytopes: what enumerate() of frx_geometry.cpp computes for one polytope on the host,
// bit for bit and verdict included, one 256-thread workgroup per task (a corridor cell, or the overlap of two consecutive cells).
//
// The host walks every plane triple a < b < c in lexicographic order, keeps the intersection points that satisfy every plane, drops all but the FIRST of the
// points that share a 1e-7 grid key, sorts the rest by key and judges the polytope (unbounded / flat).  Here:
//   a. the task's records become (unit normal, offset) planes in LDS, one lane per plane; a record that is not finite ends the task (FRX_HV_NONFINITE);
//   b. the triple list is walked in RANK order in windows of 256, lane = one triple, unranked with integer arithmetic (hv_unrank: two binary searches over
//      closed-form counts, no floating-point root); the lane forms the point and runs the feasibility loop over the planes out of LDS;
//   c. the feasible lanes of a wave stage key and point in that wave's 64 entries of LDS in lane order (ballot + prefix), so the staged entries of waves 0..3
//      read in turn ARE the window's feasible triples in rank order; a window without a feasible triple costs one barrier;
//   d. staged entry j (lane j) survives when its key is neither in the accepted list nor held by a staged entry below j, and the survivors are appended to the
//      accepted list in order (ballot + prefix again): the first triple in rank order that reaches a key owns it, with its own coordinates;
//   e. every accepted entry ranks itself by counting smaller keys (keys are unique: a permutation), the vertices leave in that order, one lane sums the
//      centroid over them in vertex order, and the workgroup runs the two verdict tests (one lane per plane pair / per plane) - both existential, so the
//      host's early exits do not make them order-dependent.
// Every operation of a. - e. that produces a number is a correctly rounded IEEE operation in the host's order with contraction off (hv_* below), as the host
// objects are built; every decision that steers a branch around a barrier (task fields, counts, flags) is read from LDS, so the whole workgroup takes it.
// All loops are bounded by K and C(K, 3); no atomics, no spins, no traffic between workgroups: a task's output depends on that task alone.
//
// Not built: an O(K^3) edge-clipping enumeration - it meets other duplicates in another order and would lose the bit-for-bit referee.
#pragma once
#include <hip/hip_runtime.h>

#include "frx_enumerate_rank.hpp"

namespace frx {

enum { HV_OK = 0, HV_UNBOUNDED = 1, HV_FLAT = 2, HV_PLANES = 3, HV_VERTICES = 4, HV_NONFINITE = 5, HV_SKIPPED = 6 };   // FRX_HV_* of include/frx.h
enum { HV_MAX_PLANES = 256, HV_MIN_CAP_V = 4, HV_MAX_CAP_V = 512, HV_WINDOW = 256 };

struct EnumArgs {
    const int *tasks;            // [n_tasks][4] = begin0, count0, begin1, count1 in records of h_rec
    const double *h_rec;         // records of 6 doubles (outer normal, point)
    int n_tasks, cap_v;
    double *v_slot;              // [n_tasks][cap_v][3]
    int *nv, *status;            // [n_tasks]
};

// hv_c3, hv_before, hv_unrank, hv_unrank_pair: frx_enumerate_rank.hpp (plain C++, checked rank by rank on the host)

// frx_geometry.cpp:42-46
__device__ __forceinline__ void hv_plane(const double *r, double *pl) {
#pragma clang fp contract(off)
    const double nn = __builtin_sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
    pl[0] = r[0] / nn; pl[1] = r[1] / nn; pl[2] = r[2] / nn; pl[3] = (r[0] * r[3] + r[1] * r[4] + r[2] * r[5]) / nn;
}

// frx_geometry.cpp:51-62: the point of planes a, b, c and whether every plane holds it
__device__ __forceinline__ bool hv_triple(const double *pl, int K, int a, int b, int c, double &x0, double &x1, double &x2) {
#pragma clang fp contract(off)
    const double *A = pl + 4 * a, *B = pl + 4 * b, *C = pl + 4 * c;
    const double A0 = A[0], A1 = A[1], A2 = A[2], A3 = A[3], B0 = B[0], B1 = B[1], B2 = B[2], B3 = B[3], C0 = C[0], C1 = C[1], C2 = C[2], C3 = C[3];
    const double cx = B1 * C2 - B2 * C1, cy = B2 * C0 - B0 * C2, cz = B0 * C1 - B1 * C0;   // B x C
    const double det = A0 * cx + A1 * cy + A2 * cz;
    if (__builtin_fabs(det) <= 1e-10) return false;
    const double ax = C1 * A2 - C2 * A1, ay = C2 * A0 - C0 * A2, az = C0 * A1 - C1 * A0;   // C x A
    const double bx = A1 * B2 - A2 * B1, by = A2 * B0 - A0 * B2, bz = A0 * B1 - A1 * B0;   // A x B
    x0 = (A3 * cx + B3 * ax + C3 * bx) / det; x1 = (A3 * cy + B3 * ay + C3 * by) / det; x2 = (A3 * cz + B3 * az + C3 * bz) / det;
    bool feas = true;
    for (int k = 0; k < K && feas; k++) feas = pl[4 * k] * x0 + pl[4 * k + 1] * x1 + pl[4 * k + 2] * x2 <= pl[4 * k + 3] + 1e-9;
    return feas;
}

// frx_geometry.cpp:69
__device__ __forceinline__ long long hv_key(double v) {
#pragma clang fp contract(off)
    return (long long)__builtin_nearbyint(v / 1e-7);
}

// frx_geometry.cpp:84-94 for one pair: sp |= some plane is not parallel to u = n_a x n_b / |n_a x n_b|, ray |= +u or -u leaves through no plane
__device__ __forceinline__ void hv_pair(const double *pl, int K, int a, int b, bool &sp, bool &ray) {
#pragma clang fp contract(off)
    const double *A = pl + 4 * a, *B = pl + 4 * b;
    double u0 = A[1] * B[2] - A[2] * B[1], u1 = A[2] * B[0] - A[0] * B[2], u2 = A[0] * B[1] - A[1] * B[0];
    const double un = __builtin_sqrt(u0 * u0 + u1 * u1 + u2 * u2);
    if (un <= 1e-10) return;
    u0 /= un; u1 /= un; u2 /= un;
    bool fneg = true, fpos = true;
    for (int k = 0; k < K && (fneg || fpos || !sp); k++) {
        const double dot = pl[4 * k] * u0 + pl[4 * k + 1] * u1 + pl[4 * k + 2] * u2;
        sp = sp || __builtin_fabs(dot) > 1e-10;
        fneg = fneg && -dot <= 1e-12;
        fpos = fpos && dot <= 1e-12;
    }
    ray = ray || fneg || fpos;
}

// frx_geometry.cpp:99-101: the centroid of the sorted vertices, summed in vertex order
__device__ __forceinline__ void hv_centroid(const double *ax, const int *perm, int cap, int nv, double *c) {
#pragma clang fp contract(off)
    double c0 = 0.0, c1 = 0.0, c2 = 0.0;
    for (int i = 0; i < nv; i++) { const int s = perm[i]; c0 += ax[s]; c1 += ax[cap + s]; c2 += ax[2 * cap + s]; }
    c[0] = c0 / (double)nv; c[1] = c1 / (double)nv; c[2] = c2 / (double)nv;
}
// frx_geometry.cpp:103-104: std::min keeps the old value when the new one is NaN, so the polytope is flat exactly when some slack compares <= 1e-9
__device__ __forceinline__ bool hv_no_slack(const double *p, const double *c) {
#pragma clang fp contract(off)
    return p[3] - (p[0] * c[0] + p[1] * c[1] + p[2] * c[2]) <= 1e-9;
}

__device__ __forceinline__ int hv_lanes_below(unsigned long long m) { return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u)); }
__device__ __forceinline__ bool hv_key_less(long long a0, long long a1, long long a2, long long b0, long long b1, long long b2) {
    return a0 != b0 ? a0 < b0 : (a1 != b1 ? a1 < b1 : a2 < b2);
}

// dynamic LDS: accepted keys [3][cap_v] (long long) | accepted points [3][cap_v] (double) | perm [cap_v] (int) = 52 cap_v bytes
__global__ __launch_bounds__(256) void k_enumerate(EnumArgs g) {
    extern __shared__ __attribute__((aligned(16))) double hv_dyn[];
    __shared__ __attribute__((aligned(16))) double pl[4 * HV_MAX_PLANES];       // 8 KB
    __shared__ long long skey[3][HV_WINDOW];                                     // a window's feasible triples: wave w stages in entries 64 w ..
    __shared__ double sx[3][HV_WINDOW];
    __shared__ double s_cen[3];
    __shared__ int s_task[4], s_bad[4], s_cnt[2][4], s_surv[4], s_sp[4], s_ray[4], s_flat[4];
    const int t = threadIdx.x, w = t >> 6, task = blockIdx.x, cap = g.cap_v;
    long long *akey = (long long *)hv_dyn;
    double *ax = hv_dyn + (size_t)3 * cap;
    int *perm = (int *)(hv_dyn + (size_t)6 * cap);

    if (t < 4) s_task[t] = g.tasks[(size_t)4 * task + t];
    __syncthreads();
    const int b0 = s_task[0], c0 = s_task[1], b1 = s_task[2], c1 = s_task[3];
    if (c0 == 0) { if (t == 0) { g.status[task] = HV_SKIPPED; g.nv[task] = 0; } return; }
    if (c0 < 0 || c1 < 0 || c0 > HV_MAX_PLANES || c1 > HV_MAX_PLANES || c0 + c1 < 4 || c0 + c1 > HV_MAX_PLANES) {
        if (t == 0) { g.status[task] = HV_PLANES; g.nv[task] = 0; }
        return;
    }
    const int K = c0 + c1;

    // ---- a. planes ----
    bool bad = false;
    if (t < K) {
        const double *rp = g.h_rec + (size_t)6 * (t < c0 ? (size_t)b0 + t : (size_t)b1 + (t - c0));
        double r[6];
#pragma unroll
        for (int i = 0; i < 6; i++) { r[i] = rp[i]; bad = bad || !__builtin_isfinite(r[i]); }
        hv_plane(r, pl + 4 * t);
    }
    const unsigned long long mb = __builtin_amdgcn_ballot_w64(bad);
    if ((t & 63) == 0) s_bad[w] = mb != 0ull;
    __syncthreads();
    if (s_bad[0] | s_bad[1] | s_bad[2] | s_bad[3]) { if (t == 0) { g.status[task] = HV_NONFINITE; g.nv[task] = 0; } return; }

    // ---- b. - d. the triples, a window of 256 ranks at a time ----
    const int total = hv_c3(K);
    int n_acc = 0;
    bool over = false;
    for (int r0 = 0, par = 0; r0 < total; r0 += HV_WINDOW, par ^= 1) {
        const int r = r0 + t;
        bool feas = false;
        double x0 = 0.0, x1 = 0.0, x2 = 0.0;
        if (r < total) { int a, b, c; hv_unrank(K, r, a, b, c); feas = hv_triple(pl, K, a, b, c, x0, x1, x2); }
        const unsigned long long mf = __builtin_amdgcn_ballot_w64(feas);
        if (feas) {
            const int e = 64 * w + hv_lanes_below(mf);
            skey[0][e] = hv_key(x0); skey[1][e] = hv_key(x1); skey[2][e] = hv_key(x2);
            sx[0][e] = x0; sx[1][e] = x1; sx[2][e] = x2;
        }
        if ((t & 63) == 0) s_cnt[par][w] = __popcll(mf);
        __syncthreads();
        const int n0 = s_cnt[par][0], n1 = s_cnt[par][1], n2 = s_cnt[par][2], n3 = s_cnt[par][3], nf = n0 + n1 + n2 + n3;
        if (nf == 0) continue;
        // staged entry j = t, in rank order: wave 0's entries, then wave 1's, ...
        bool surv = false;
        long long k0 = 0, k1 = 0, k2 = 0;
        if (t < nf) {
            int jw = 0, ji = t;
            if (ji >= n0) { ji -= n0; jw = 1; if (ji >= n1) { ji -= n1; jw = 2; if (ji >= n2) { ji -= n2; jw = 3; } } }
            const int e = 64 * jw + ji;
            k0 = skey[0][e]; k1 = skey[1][e]; k2 = skey[2][e]; x0 = sx[0][e]; x1 = sx[1][e]; x2 = sx[2][e];
            bool seen = false;
            for (int i = 0; i < n_acc && !seen; i++) seen = akey[i] == k0 && akey[cap + i] == k1 && akey[2 * cap + i] == k2;
            for (int ww = 0; ww <= jw && !seen; ww++) {
                const int lim = ww < jw ? s_cnt[par][ww] : ji;
                for (int i = 0; i < lim && !seen; i++) seen = skey[0][64 * ww + i] == k0 && skey[1][64 * ww + i] == k1 && skey[2][64 * ww + i] == k2;
            }
            surv = !seen;
        }
        const unsigned long long ms = __builtin_amdgcn_ballot_w64(surv);
        if ((t & 63) == 0) s_surv[w] = __popcll(ms);
        __syncthreads();
        const int q0 = s_surv[0], q1 = s_surv[1], q2 = s_surv[2], q3 = s_surv[3], ns = q0 + q1 + q2 + q3;
        if (n_acc + ns > cap) { over = true; break; }
        if (surv) {
            const int p = n_acc + (w > 0 ? q0 : 0) + (w > 1 ? q1 : 0) + (w > 2 ? q2 : 0) + hv_lanes_below(ms);
            akey[p] = k0; akey[cap + p] = k1; akey[2 * cap + p] = k2;
            ax[p] = x0; ax[cap + p] = x1; ax[2 * cap + p] = x2;
        }
        n_acc += ns;
    }
    if (over) { if (t == 0) { g.status[task] = HV_VERTICES; g.nv[task] = 0; } return; }
    __syncthreads();

    // ---- e. order ----
    const int nv = n_acc;
    for (int i = t; i < nv; i += 256) {
        const long long a0 = akey[i], a1 = akey[cap + i], a2 = akey[2 * cap + i];
        int rk = 0;
        for (int j = 0; j < nv; j++) rk += hv_key_less(akey[j], akey[cap + j], akey[2 * cap + j], a0, a1, a2) ? 1 : 0;
        perm[rk] = i;
    }
    __syncthreads();
    double *vs = g.v_slot + (size_t)task * cap * 3;
    for (int i = t; i < nv; i += 256) { const int s = perm[i]; vs[3 * i] = ax[s]; vs[3 * i + 1] = ax[cap + s]; vs[3 * i + 2] = ax[2 * cap + s]; }

    // ---- verdict ----
    bool sp = false, ray = false;
    const int npairs = K * (K - 1) / 2;
    for (int p = t; p < npairs; p += 256) { int a, b; hv_unrank_pair(K, p, a, b); hv_pair(pl, K, a, b, sp, ray); }
    const unsigned long long msp = __builtin_amdgcn_ballot_w64(sp), mray = __builtin_amdgcn_ballot_w64(ray);
    if ((t & 63) == 0) { s_sp[w] = msp != 0ull; s_ray[w] = mray != 0ull; }
    if (t == 0 && nv >= 4) hv_centroid(ax, perm, cap, nv, s_cen);
    __syncthreads();
    bool noslack = false;
    if (nv >= 4 && t < K) noslack = hv_no_slack(pl + 4 * t, s_cen);
    const unsigned long long mfl = __builtin_amdgcn_ballot_w64(noslack);
    if ((t & 63) == 0) s_flat[w] = mfl != 0ull;
    __syncthreads();
    if (t == 0) {
        const bool spans = s_sp[0] | s_sp[1] | s_sp[2] | s_sp[3], anyray = s_ray[0] | s_ray[1] | s_ray[2] | s_ray[3];
        const bool flat = nv < 4 || (s_flat[0] | s_flat[1] | s_flat[2] | s_flat[3]);
        g.status[task] = (!spans || anyray) ? HV_UNBOUNDED : (flat ? HV_FLAT : HV_OK);
        g.nv[task] = nv;
    }
}

// tasks of the corridor generator's slots (frx_corridor_generate_batch_device): position i of path p is cell i / 2 (i even) or the overlap of cells i / 2 and
// i / 2 + 1 (i odd); record indices into h_slot [n_paths][cap_polys][cap_planes] viewed as one record array; positions beyond the path's cells: count0 = 0
__global__ __launch_bounds__(256) void k_slots_to_tasks(int n_paths, int cap_polys, int cap_planes, const int *cell_planes, const int *n_polys, int *tasks) {
    const int per = 2 * cap_polys - 1;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)n_paths * per) return;
    const int p = (int)(i / per), q = (int)(i % per), c = q >> 1, np = n_polys[p];
    int o0 = 0, o1 = 0, o2 = 0, o3 = 0;
    const size_t cell = (size_t)p * cap_polys + c;
    if ((q & 1) == 0 && c < np) { o0 = (int)(cell * cap_planes); o1 = cell_planes[cell]; }
    if ((q & 1) == 1 && c + 1 < np) { o0 = (int)(cell * cap_planes); o1 = cell_planes[cell]; o2 = (int)((cell + 1) * cap_planes); o3 = cell_planes[cell + 1]; }
    int *o = tasks + 4 * i;
    o[0] = o0; o[1] = o1; o[2] = o2; o[3] = o3;
}

} // namespace frx
