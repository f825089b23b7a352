// TEST INFRASTRUCTURE (not part of the default build, never loaded into Python):
//  - a stand-alone host program meant for a sanitizer build (make -C fast-racing_amd/csrc esdf_san && tests/hostcheck/esdf_san): the host form of the voxel map's distance field
//    (frx_esdf_host.hpp: the integer lower envelope, the square roots, the combine rule) over random small maps, each against the definition - the minimum
//    over all pairs (cell, site) - and the plan header (frx_esdf_plan.hpp) over a grid of dimensions against its stated rules.  Under the address and
//    undefined-behaviour sanitizers an index past a line's stack, a signed overflow in a squared distance or a plan's size stops the run.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "../../fast-racing_amd/csrc/frx_esdf_host.hpp"

static int brute(const std::vector<signed char> &cells, const int *dim, bool occupied, int x, int y, int z) {
    long long best = frx::ESDF_INF;
    for (int k = 0; k < dim[2]; k++)
        for (int j = 0; j < dim[1]; j++)
            for (int i = 0; i < dim[0]; i++) {
                const signed char c = cells[(size_t)i + (size_t)dim[0] * j + (size_t)dim[0] * dim[1] * k];
                if (occupied ? c > 0 : c == 0) {
                    const long long d = (long long)(i - x) * (i - x) + (long long)(j - y) * (j - y) + (long long)(k - z) * (k - z);
                    if (d < best) best = d;
                }
            }
    return (int)best;
}

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

int main() {
    std::mt19937_64 rng(7);
    long long maps = 0, cells_checked = 0;
    const signed char values[5] = {-1, 0, 1, 99, 100};
    for (int trial = 0; trial < 400; trial++) {
        int dim[3];
        for (int a = 0; a < 3; a++) dim[a] = 1 + (int)(rng() % (trial % 7 == 0 ? 23 : 8));
        const size_t n = (size_t)dim[0] * dim[1] * dim[2];
        std::vector<signed char> cells(n);
        const int kind = trial % 6;                                       // all unknown, all free, all occupied, sparse, dense, every value
        for (size_t c = 0; c < n; c++)
            cells[c] = kind == 0 ? -1 : kind == 1 ? 0 : kind == 2 ? 100 : kind == 3 ? (rng() % 50 == 0 ? 100 : 0) : kind == 4 ? (rng() % 3 ? 100 : -1) : values[rng() % 5];
        const double res = trial % 2 ? 0.1 : 0.3;
        std::vector<double> pos(n), neg(n), all(n), only(n);
        frx::esdf_host(cells.data(), dim, res, pos.data(), neg.data(), all.data());
        frx::esdf_host(cells.data(), dim, res, nullptr, nullptr, only.data());
        for (int z = 0; z < dim[2]; z++)
            for (int y = 0; y < dim[1]; y++)
                for (int x = 0; x < dim[0]; x++) {
                    const size_t c = (size_t)x + (size_t)dim[0] * y + (size_t)dim[0] * dim[1] * z;
                    const double p = frx::esdf_metres(brute(cells, dim, true, x, y, z), res), m = frx::esdf_metres(brute(cells, dim, false, x, y, z), res);
                    const double a = frx::esdf_combine(p, m, res);
                    if (!same_bits(pos[c], p) || !same_bits(neg[c], m) || !same_bits(all[c], a) || !same_bits(only[c], a)) {
                        std::printf("MISMATCH trial %d dim %d %d %d cell %d %d %d: pos %.17g / %.17g neg %.17g / %.17g all %.17g / %.17g\n", trial, dim[0], dim[1], dim[2], x, y,
                                    z, pos[c], p, neg[c], m, all[c], a);
                        return 1;
                    }
                    cells_checked++;
                }
        maps++;
    }
    // a line at the limits: the largest squared distances stay inside an int
    {
        const int dim[3] = {1, frx::ESDF_MAX_DIM, 1};
        std::vector<signed char> cells(frx::ESDF_MAX_DIM, 0);
        cells[0] = 100;
        std::vector<double> pos(frx::ESDF_MAX_DIM);
        frx::esdf_host(cells.data(), dim, 1.0, pos.data(), nullptr, nullptr);
        if (pos[frx::ESDF_MAX_DIM - 1] != (double)(frx::ESDF_MAX_DIM - 1)) { std::printf("MISMATCH at the end of the longest line: %.17g\n", pos[frx::ESDF_MAX_DIM - 1]); return 1; }
    }
    // the plan over a grid of dimensions
    long long plans = 0;
    const int vals[] = {-1, 0, 1, 2, 255, 256, 257, 4096, frx::ESDF_MAX_LINE, frx::ESDF_MAX_LINE + 1, frx::ESDF_MAX_DIM, frx::ESDF_MAX_DIM + 1, 0x7fffffff};
    for (int a : vals)
        for (int b : vals)
            for (int c : vals) {
                const int dim[3] = {a, b, c};
                const frx::EsdfPlan p = frx::esdf_plan(dim);
                const bool invalid = a <= 0 || b <= 0 || c <= 0;
                const double cells = (double)a * b * c;
                const bool capacity = !invalid && (a > frx::ESDF_MAX_LINE || b > frx::ESDF_MAX_DIM || c > frx::ESDF_MAX_DIM || cells > 2147483647.0);
                const frx::EsdfVerdict want = invalid ? frx::ESDF_INVALID : capacity ? frx::ESDF_CAPACITY : frx::ESDF_FITS;
                bool ok = p.verdict == want;
                if (ok && want == frx::ESDF_FITS)
                    ok = p.cells == (long long)cells && p.work_bytes == 4 * (4 * (size_t)p.cells + (size_t)a + 1 + 2 * (size_t)p.columns) && (long long)p.grid_ycol * frx::ESDF_THREADS >= a && (long long)p.grid_z * frx::ESDF_THREADS >= p.columns &&
                         (long long)p.grid_y * frx::ESDF_THREADS >= p.cells && (long long)(p.grid_y - 1) * frx::ESDF_THREADS < p.cells && p.grid_x == (unsigned)b * (unsigned)c &&
                         p.lds_x == 8u * (unsigned)a && p.lds_x <= 64u * 1024u && (long long)p.grid_flags * frx::ESDF_THREADS >= a + 1;
                if (!ok) { std::printf("PLAN MISMATCH dim %d %d %d: verdict %d, wanted %d\n", a, b, c, (int)p.verdict, (int)want); return 1; }
                plans++;
            }
    std::printf("esdf: %lld maps, %lld cells against the definition, %lld plans: 0 mismatches\n", maps, cells_checked, plans);
    return 0;
}
