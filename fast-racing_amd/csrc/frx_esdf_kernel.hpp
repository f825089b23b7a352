// The distance field of a voxel map on the device (frx_map_esdf_device, include/frx.h; MapUtil::updateESDF3d, map_util.h:149-245) and frx_map_mark_cloud on the
// device (setObs, map_util.h:108-136).  The host form (frx_esdf_host.hpp) finds each line's lower envelope of parabolas; that walk is serial along a line and needs
// a stack per line.  Here every pass is a search per cell instead, exact for the same reason the envelope is - the values are integers below 2^31
// (frx_esdf_plan.hpp) - and with no stack, no atomics on the values and no order of reduction: the field is bit-identical run to run and to the host's.
//
//   k_esdf_flags   zeroes the nx + 1 flag words.
//   k_esdf_z       one lane per (x, y) column, columns flat so that every load coalesces whatever nx is.  The input is binary, so one sweep up the column and
//                  one down give dz^2 towards the nearest occupied and the nearest free cell.  A column with a site sets its bit (1 occupied, 2 free) in flag[x]
//                  and in flag[nx] with a vector atomic OR - an OR has no order; a word that already holds the bit is left alone.
//   k_esdf_ycol    one lane per x.  Along y the finite entries of a line (x, ., z) stand exactly at the columns (x, y) that hold a site, whatever z is: a sweep
//                  along y and one back over the nx ny columns leave, per column, the distance to the nearest such column.
//   k_esdf_y       one lane per cell, cells flat.  best = g[q]; for d = 1, 2, ...: stop once d^2 >= best or both ends of the line are passed;
//                  best = min(best, g[q -+ d] + d^2), the sentinel tested before the add.  A line (x, ., z) holds a site exactly when flag[x] has the bit: without
//                  it the cell is ESDF_INF at once, where the search would walk the whole line for nothing (ny^2 per line on an empty map).  With it the walk STARTS at
//                  the column's distance d0 - everything nearer is ESDF_INF - and ends within about dz^2 / (2 d0) further steps: its work does not grow with d0.
//   k_esdf_x       one workgroup per x line: the line of both site sets is staged in LDS (8 bytes a cell) and searched there in the same way; flag[nx] says
//                  whether any site exists at all.  It then writes the doubles: res sqrt(d2), +inf without a site, and the combined field with pos rounded
//                  before it enters the sum - the whole translation unit is built without contraction, as map_blocked is.
// The x pass has no such start: the work of its search is the distance it finds, in LDS.  DESIGN 3.20 has the figures.
#pragma once
#include <hip/hip_runtime.h>

#include "frx_esdf_plan.hpp"

namespace frx {

struct EsdfArgs {
    const signed char *cells;            // [nz][ny][nx]
    int nx, ny, nz, ncol, n;             // ncol = nx ny, n = ncol nz
    double res;
    int *gz_occ, *gz_free, *gy_occ, *gy_free, *flag;   // the workspace: four [n] arrays, then nx + 1 words,
    int *yd_occ, *yd_free;               // then two [ncol] arrays: the distance along y to the nearest column with a site
    int want_occ, want_free;             // which site sets an output needs
    double *pos, *neg, *all;             // outputs, each may be null
};

__global__ void __launch_bounds__(ESDF_THREADS) k_esdf_flags(int *flag, int words) {
    const int i = blockIdx.x * ESDF_THREADS + threadIdx.x;
    if (i < words) flag[i] = 0;
}

__device__ __forceinline__ void esdf_set_flag(int *word, int bits) {
    if ((__atomic_load_n(word, __ATOMIC_RELAXED) & bits) != bits) atomicOr(word, bits);
}

__global__ void __launch_bounds__(ESDF_THREADS) k_esdf_z(EsdfArgs a) {
    const int col = blockIdx.x * ESDF_THREADS + threadIdx.x;
    if (col >= a.ncol) return;
    const signed char *c = a.cells + col;
    int *go = a.gz_occ + col, *gf = a.gz_free + col;
    int d_occ = -1, d_free = -1;                                          // cells since the last site, -1 before the first
    for (int z = 0; z < a.nz; z++) {
        const size_t o = (size_t)z * a.ncol;
        const int v = c[o];
        d_occ = v > 0 ? 0 : d_occ < 0 ? -1 : d_occ + 1;
        d_free = v == 0 ? 0 : d_free < 0 ? -1 : d_free + 1;
        if (a.want_occ) go[o] = d_occ < 0 ? (int)ESDF_INF : d_occ * d_occ;
        if (a.want_free) gf[o] = d_free < 0 ? (int)ESDF_INF : d_free * d_free;
    }
    int bits = 0;
    d_occ = -1; d_free = -1;
    for (int z = a.nz - 1; z >= 0; z--) {
        const size_t o = (size_t)z * a.ncol;
        const int v = c[o];
        d_occ = v > 0 ? 0 : d_occ < 0 ? -1 : d_occ + 1;
        d_free = v == 0 ? 0 : d_free < 0 ? -1 : d_free + 1;
        if (v > 0) bits |= 1;
        if (v == 0) bits |= 2;
        if (a.want_occ && d_occ >= 0 && d_occ * d_occ < go[o]) go[o] = d_occ * d_occ;
        if (a.want_free && d_free >= 0 && d_free * d_free < gf[o]) gf[o] = d_free * d_free;
    }
    a.yd_occ[col] = (bits & 1) ? 0 : (int)ESDF_INF;
    a.yd_free[col] = (bits & 2) ? 0 : (int)ESDF_INF;
    if (bits) {
        esdf_set_flag(a.flag + col % a.nx, bits);
        esdf_set_flag(a.flag + a.nx, bits);
    }
}

// one lane per x: the columns (x, .) hold 0 (a site) or ESDF_INF; a sweep along y and one back leave the distance in cells to the nearest column with a site.
// A sweep is a chain of ny steps on few lanes, so it is bound by the latency of its loads: both site sets run side by side and ESDF_YCHUNK entries of each are
// loaded before the first of them is used or stored, which puts that many loads in flight at once.  UP: y ascending, else descending.
static constexpr int ESDF_YCHUNK = 16;
template <bool UP>
__device__ __forceinline__ void esdf_column_sweep(int *__restrict__ yo, int *__restrict__ yf, int nx, int ny) {
    int d_o = -1, d_f = -1;                                               // columns since the last site, -1 before the first
    for (int y0 = 0; y0 < ny; y0 += ESDF_YCHUNK) {
        int vo[ESDF_YCHUNK], vf[ESDF_YCHUNK];
#pragma unroll
        for (int k = 0; k < ESDF_YCHUNK; k++) {
            const int s = y0 + k, y = UP ? s : ny - 1 - s;
            vo[k] = s < ny ? yo[(size_t)y * nx] : 0;
            vf[k] = s < ny ? yf[(size_t)y * nx] : 0;
        }
#pragma unroll
        for (int k = 0; k < ESDF_YCHUNK; k++) {
            const int s = y0 + k, y = UP ? s : ny - 1 - s;
            if (s < ny) {                                                 // (the last chunk may reach past the line)
                d_o = vo[k] == 0 ? 0 : d_o < 0 ? -1 : d_o + 1;            // (0 stands at the sites alone: a sweep writes distances above 0)
                d_f = vf[k] == 0 ? 0 : d_f < 0 ? -1 : d_f + 1;
                if (d_o > 0 && d_o < vo[k]) yo[(size_t)y * nx] = d_o;
                if (d_f > 0 && d_f < vf[k]) yf[(size_t)y * nx] = d_f;
            }
        }
    }
}
__global__ void __launch_bounds__(ESDF_THREADS) k_esdf_ycol(EsdfArgs a) {
    const int x = blockIdx.x * ESDF_THREADS + threadIdx.x;
    if (x >= a.nx) return;
    esdf_column_sweep<true>(a.yd_occ + x, a.yd_free + x, a.nx, a.ny);
    esdf_column_sweep<false>(a.yd_occ + x, a.yd_free + x, a.nx, a.ny);
}

// the search along a line: g(i) reads entry i of the line, q the cell, len the line's length; every entry nearer than `start` is known to be ESDF_INF
template <class Get>
__device__ __forceinline__ int esdf_search(Get g, int q, int len, int start = 1) {
    int best = g(q);
    for (int d = start;; d++) {
        const int dd = d * d;
        if (dd >= best) break;                                            // (best = ESDF_INF: never, the ends stop the walk)
        const bool lo = q - d >= 0, hi = q + d < len;
        if (!lo && !hi) break;
        if (lo) { const int v = g(q - d); if (v != ESDF_INF && v + dd < best) best = v + dd; }
        if (hi) { const int v = g(q + d); if (v != ESDF_INF && v + dd < best) best = v + dd; }
    }
    return best;
}

__global__ void __launch_bounds__(ESDF_THREADS) k_esdf_y(EsdfArgs a) {
    const long long i = (long long)blockIdx.x * ESDF_THREADS + threadIdx.x;
    if (i >= a.n) return;
    const int x = (int)(i % a.nx), y = (int)(i / a.nx % a.ny);
    const int bits = a.flag[x];
    const size_t base = (size_t)i - (size_t)y * a.nx;                     // entry 0 of the cell's line
    const int col = x + a.nx * y;
    if (a.want_occ) {
        const int *g = a.gz_occ + base;
        const int d0 = a.yd_occ[col];
        a.gy_occ[i] = (bits & 1) ? esdf_search([&](int k) { return g[(size_t)k * a.nx]; }, y, a.ny, d0 > 1 ? d0 : 1) : (int)ESDF_INF;
    }
    if (a.want_free) {
        const int *g = a.gz_free + base;
        const int d0 = a.yd_free[col];
        a.gy_free[i] = (bits & 2) ? esdf_search([&](int k) { return g[(size_t)k * a.nx]; }, y, a.ny, d0 > 1 ? d0 : 1) : (int)ESDF_INF;
    }
}

__global__ void __launch_bounds__(ESDF_THREADS) k_esdf_x(EsdfArgs a) {
#pragma clang fp contract(off)
    extern __shared__ int esdf_lds[];
    int *lo = esdf_lds, *lf = esdf_lds + a.nx;
    const size_t base = (size_t)blockIdx.x * a.nx;
    const int bits = a.flag[a.nx];
    for (int x = threadIdx.x; x < a.nx; x += ESDF_THREADS) {
        if (a.want_occ) lo[x] = a.gy_occ[base + x];
        if (a.want_free) lf[x] = a.gy_free[base + x];
    }
    __syncthreads();
    const double inf = __builtin_huge_val();
    for (int x = threadIdx.x; x < a.nx; x += ESDF_THREADS) {
        double p = 0.0, m = 0.0;
        if (a.want_occ) {
            const int d2 = (bits & 1) ? esdf_search([&](int k) { return lo[k]; }, x, a.nx) : (int)ESDF_INF;
            p = d2 == ESDF_INF ? inf : a.res * sqrt((double)d2);
        }
        if (a.want_free) {
            const int d2 = (bits & 2) ? esdf_search([&](int k) { return lf[k]; }, x, a.nx) : (int)ESDF_INF;
            m = d2 == ESDF_INF ? inf : a.res * sqrt((double)d2);
        }
        if (a.pos) a.pos[base + x] = p;
        if (a.neg) a.neg[base + x] = m;
        if (a.all) {
            double v = p;
            if (m > 0.0) v += (-m + a.res);                               // map_util.h:241-243, the parenthesis first
            a.all[base + x] = v != v ? __builtin_nan("") : v;             // (inf - inf: the plain quiet NaN, as the host writes it)
        }
    }
}

// ---- frx_map_mark_cloud on the device ----
struct MarkArgs {
    double origin[3], res;
    int dim[3];
    signed char *cells;
    const double *pts;
    int n_pts;
    int *n_inside;
};

__global__ void k_mark_zero(int *n_inside) { *n_inside = 0; }

// one lane per point; map_blocked's cell rule (frx_chain_kernel.hpp), none of it fused.  The comparison is made on the rounded double, so a point far outside or
// not a number is outside, as the host's conversion makes it.  Racing byte stores all write 100; the count is one vector integer atomic per wave.
__global__ void __launch_bounds__(ESDF_THREADS) k_mark_cloud(MarkArgs a) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * ESDF_THREADS + threadIdx.x;
    bool inside = false;
    if (i < a.n_pts) {
        const double *p = a.pts + 3 * (size_t)i;
        const double cx = round((p[0] - a.origin[0]) / a.res - 0.5), cy = round((p[1] - a.origin[1]) / a.res - 0.5), cz = round((p[2] - a.origin[2]) / a.res - 0.5);
        inside = cx >= 0.0 && cx < (double)a.dim[0] && cy >= 0.0 && cy < (double)a.dim[1] && cz >= 0.0 && cz < (double)a.dim[2];
        if (inside) a.cells[(size_t)(int)cx + (size_t)a.dim[0] * (size_t)(int)cy + (size_t)a.dim[0] * a.dim[1] * (size_t)(int)cz] = 100;
    }
    const unsigned long long mask = __ballot(inside);
    if ((threadIdx.x & 63) == 0 && mask) atomicAdd(a.n_inside, __popcll(mask));
}

} // namespace frx
