// The distance field of a voxel map on the host (frx_map_esdf, include/frx.h): MapUtil::updateESDF3d / fillESDF (map_util.h:149-278) with integer values.
// Plain C++ on one thread; frx_search.cpp wraps it and tests/hostcheck/esdf_main.cpp runs it under the sanitizers.  It is the referee of the device form
// (frx_esdf_kernel.hpp), which finds the same integers by another method.
//
// The reference keeps squared distances as doubles with DBL_MAX for "no site" and finds each line's lower envelope of parabolas from intersection points
// s = ((f(q) + q^2) - (f(v) + v^2)) / (2q - 2v).  The values are integers below 2^31 (frx_esdf_plan.hpp), so here the envelope is kept over the finite sites only
// and an intersection is the first INTEGER at which the later parabola is strictly lower, floor(s) + 1 in 64-bit integers: no rounding anywhere, and a line
// without a site stays ESDF_INF.  Must be compiled without floating-point contraction (the combine rule rounds pos before the sum).
#pragma once
#include <cmath>
#include <cstdint>
#include <limits>
#include <vector>

#include "frx_esdf_plan.hpp"

namespace frx {

// One line of n values at g[0], g[stride], ...: out[i stride] = min over q with g finite of g[q] + (i - q)^2, ESDF_INF when there is none.  v, fv (the envelope's
// sites and their values, copied out so that out may be g) hold n entries, z (the first integer of each site's stretch) n + 1.
inline void esdf_line(const int *g, int *out, int n, size_t stride, int *v, long long *z, int *fv) {
    int k = -1;
    for (int q = 0; q < n; q++) {
        const long long fq = g[q * stride];
        if (fq == ESDF_INF) continue;
        long long s = std::numeric_limits<long long>::min();
        while (k >= 0) {
            const long long a = (fq + (long long)q * q) - ((long long)fv[k] + (long long)v[k] * v[k]), b = 2LL * q - 2LL * v[k];
            long long fl = a / b;
            if (a % b != 0 && a < 0) fl--;                               // floor, not truncation
            s = fl + 1;
            if (s > z[k]) break;
            k--;
        }
        if (k < 0) s = std::numeric_limits<long long>::min();
        k++;
        v[k] = q; z[k] = s; fv[k] = (int)fq;
    }
    if (k < 0) {
        for (int i = 0; i < n; i++) out[i * stride] = ESDF_INF;
        return;
    }
    const int last = k;
    k = 0;
    for (int i = 0; i < n; i++) {
        while (k < last && z[k + 1] <= i) k++;
        const long long d = i - v[k];
        out[i * stride] = (int)(d * d + fv[k]);
    }
}

// res sqrt(d2) of a squared distance in cells; ESDF_INF = no site at all = +inf (the reference's DBL_MAX arithmetic gives res sqrt(DBL_MAX) there)
inline double esdf_metres(int d2, double res) { return d2 == ESDF_INF ? std::numeric_limits<double>::infinity() : res * std::sqrt((double)d2); }
// map_util.h:241-243: all = pos, and where neg > 0, all += (-neg + res) with the parenthesis first.  inf - inf (no site of either kind) is not a number, and
// which one is the machine's choice - x86 sets the sign bit, gfx950 does not - so that case is written as the plain quiet NaN
inline double esdf_combine(double pos, double neg, double res) {
    double all = pos;
    if (neg > 0.0) all += (-neg + res);
    return all != all ? std::numeric_limits<double>::quiet_NaN() : all;
}

// d2[c] = squared distance in cells from cell c to the nearest site, x fastest; site(value of the cell) says which cells are sites.  d2 holds dim[0] dim[1] dim[2] ints.
template <class Site>
inline void esdf_squared(const signed char *cells, const int *dim, Site site, int *d2) {
    const int nx = dim[0], ny = dim[1], nz = dim[2];
    const size_t ncol = (size_t)nx * ny, n = ncol * nz;
    const int longest = nx > ny ? (nx > nz ? nx : nz) : (ny > nz ? ny : nz);
    std::vector<int> v(longest), fv(longest);
    std::vector<long long> z(longest + 1);
    for (size_t c = 0; c < n; c++) d2[c] = site(cells[c]) ? 0 : ESDF_INF;
    for (size_t col = 0; col < ncol; col++) esdf_line(d2 + col, d2 + col, nz, ncol, v.data(), z.data(), fv.data());                          // z (:154-167)
    for (int zc = 0; zc < nz; zc++)
        for (int x = 0; x < nx; x++) esdf_line(d2 + x + ncol * zc, d2 + x + ncol * zc, ny, (size_t)nx, v.data(), z.data(), fv.data());      // y (:169-175)
    for (size_t line = 0; line < (size_t)ny * nz; line++) esdf_line(d2 + line * nx, d2 + line * nx, nx, 1, v.data(), z.data(), fv.data());  // x (:177-185)
}

// pos, neg, all over the map (any may be null and is then not computed); the caller has accepted dim with esdf_plan
inline void esdf_host(const signed char *cells, const int *dim, double res, double *pos, double *neg, double *all) {
    const size_t n = (size_t)dim[0] * dim[1] * dim[2];
    std::vector<int> occ, fre;
    if (pos || all) { occ.resize(n); esdf_squared(cells, dim, [](signed char c) { return c > 0; }, occ.data()); }       // isOccupied (:326)
    if (neg || all) { fre.resize(n); esdf_squared(cells, dim, [](signed char c) { return c == 0; }, fre.data()); }      // isFree (:322)
    for (size_t c = 0; c < n; c++) {
        const double p = (pos || all) ? esdf_metres(occ[c], res) : 0.0, m = (neg || all) ? esdf_metres(fre[c], res) : 0.0;
        if (pos) pos[c] = p;
        if (neg) neg[c] = m;
        if (all) all[c] = esdf_combine(p, m, res);
    }
}

} // namespace frx
