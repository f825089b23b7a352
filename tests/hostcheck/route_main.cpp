// The level search of the route batch (csrc/frx_route_host.hpp) under the address and undefined-behaviour sanitizers: random small maps against a brute-force
// definition.  Distances to the goal come from repeated relaxation over the whole grid until nothing changes; then every property of the path is checked: it
// starts at the start, ends at the goal, moves by face neighbours through traversable cells, holds distance + 1 cells, and each step is the neighbour one level
// down with the smallest squared distance to the goal, first in the order -x, -y, -z, +z, +y, +x.  The level sizes, the three verdicts of the capacities and the
// workspace layout are checked as well, and the rule of a leg's end (route_end_cell) on inputs far outside, infinite and not a number.  Host code only: a
// program of its own, never loaded into Python and never run on a GPU machine (make -C fast-racing_amd/csrc route_san && tests/hostcheck/route_san).
#include <cstdio>
#include <cmath>
#include <cstdlib>
#include <limits>
#include <random>
#include <vector>

#include "../../fast-racing_amd/csrc/frx_route_host.hpp"

namespace {

int failures = 0;
#define CHECK(cond, ...)                                                  \
    do {                                                                  \
        if (!(cond)) {                                                    \
            if (failures++ < 20) { std::printf("FAILED %s:%d %s  ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
        }                                                                 \
    } while (0)

struct Grid {
    int dim[3];
    std::vector<signed char> cells;
    int id(int x, int y, int z) const { return x + dim[0] * y + dim[0] * dim[1] * z; }
    bool inside(int x, int y, int z) const { return x >= 0 && x < dim[0] && y >= 0 && y < dim[1] && z >= 0 && z < dim[2]; }
};

// distance to g by relaxation: d[c] = min over face neighbours n of d[n] + 1, swept until a sweep changes nothing
std::vector<int> relax(const Grid &G, const int *g) {
    const int INF = 1 << 30;
    std::vector<int> d(G.cells.size(), INF);
    d[G.id(g[0], g[1], g[2])] = 0;
    for (bool changed = true; changed;) {
        changed = false;
        for (int z = 0; z < G.dim[2]; z++)
            for (int y = 0; y < G.dim[1]; y++)
                for (int x = 0; x < G.dim[0]; x++) {
                    const int c = G.id(x, y, z);
                    if (G.cells[c] > 0) continue;
                    for (int k = 0; k < 6; k++) {
                        const int X = x + frx::ROUTE_STEP[k][0], Y = y + frx::ROUTE_STEP[k][1], Z = z + frx::ROUTE_STEP[k][2];
                        if (!G.inside(X, Y, Z)) continue;
                        const int n = G.id(X, Y, Z);
                        if (d[n] < INF && d[n] + 1 < d[c]) { d[c] = d[n] + 1; changed = true; }
                    }
                }
    }
    return d;
}

void one_map(std::mt19937 &rng, frx::RouteScratch &w) {
    Grid G;
    G.dim[0] = 1 + (int)(rng() % 9); G.dim[1] = 1 + (int)(rng() % 9); G.dim[2] = 1 + (int)(rng() % 4);
    const int n = G.dim[0] * G.dim[1] * G.dim[2];
    G.cells.resize(n);
    const unsigned occ = rng() % 45;
    for (auto &c : G.cells) { const unsigned r = rng() % 100; c = r < occ ? 100 : (r < occ + 5 ? -1 : 0); }
    std::vector<int> raw;
    for (int trial = 0; trial < 6; trial++) {
        int s[3], g[3];
        for (int i = 0; i < 3; i++) { s[i] = (int)(rng() % G.dim[i]); g[i] = (int)(rng() % G.dim[i]); }
        if (G.cells[G.id(s[0], s[1], s[2])] > 0 || G.cells[G.id(g[0], g[1], g[2])] > 0) continue;      // the callers check the ends
        const std::vector<int> d = relax(G, g);
        const int D = d[G.id(s[0], s[1], s[2])];
        // the sizes of the levels 0 .. min(D, last non-empty)
        std::vector<int> size;
        for (int c = 0; c < n; c++)
            if (d[c] < (1 << 30)) { if ((int)size.size() <= d[c]) size.resize(d[c] + 1, 0); size[d[c]]++; }
        const bool reach = D < (1 << 30);
        int biggest = 0;
        for (int L = 0; L < (int)size.size() && (!reach || L <= D); L++) biggest = size[L] > biggest ? size[L] : biggest;
        const frx::RouteSearchOut o = frx::route_search(G.cells.data(), G.dim, s, g, 0, 0, w, raw);
        CHECK(o.max_level_cells == biggest, "max level %d, want %d", o.max_level_cells, biggest);
        for (const unsigned char b : w.label) CHECK(b == 0, "labels not cleared");
        if (!reach) {
            CHECK(o.status == frx::ROUTE_NO_PATH && o.levels == -1 && raw.empty(), "status %d", o.status);
            continue;
        }
        CHECK(o.status == frx::ROUTE_OK && o.levels == D && (int)raw.size() == D + 1, "status %d levels %d want %d", o.status, o.levels, D);
        if (o.status != frx::ROUTE_OK || (int)raw.size() != D + 1) continue;
        CHECK(raw.front() == G.id(s[0], s[1], s[2]) && raw.back() == G.id(g[0], g[1], g[2]), "ends");
        for (int i = 0; i + 1 < (int)raw.size(); i++) {
            const int c = raw[i], x = c % G.dim[0], y = (c / G.dim[0]) % G.dim[1], z = c / (G.dim[0] * G.dim[1]);
            CHECK(G.cells[c] <= 0 && d[c] == D - i, "cell %d of the path", i);
            int best = -1;
            long long best_d = 0;
            for (int k = 0; k < 6; k++) {
                const int X = x + frx::ROUTE_STEP[k][0], Y = y + frx::ROUTE_STEP[k][1], Z = z + frx::ROUTE_STEP[k][2];
                if (!G.inside(X, Y, Z) || d[G.id(X, Y, Z)] != D - i - 1) continue;
                const long long ax = X - g[0], ay = Y - g[1], az = Z - g[2], dd = ax * ax + ay * ay + az * az;
                if (best < 0 || dd < best_d) { best = G.id(X, Y, Z); best_d = dd; }
            }
            CHECK(raw[i + 1] == best, "step %d goes to %d, the rule says %d", i, raw[i + 1], best);
        }
        // the capacities: exact, and a refused search leaves no path
        std::vector<int> r2;
        frx::RouteSearchOut c = frx::route_search(G.cells.data(), G.dim, s, g, biggest, D + 1, w, r2);
        CHECK(c.status == frx::ROUTE_OK && r2 == raw, "at the exact capacities");
        if (biggest > 1) {
            c = frx::route_search(G.cells.data(), G.dim, s, g, biggest - 1, D + 1, w, r2);
            CHECK(c.status == frx::ROUTE_CAP_LEVEL && c.levels == -1 && r2.empty(), "cap_level one short: status %d", c.status);
        }
        if (D >= 1) {
            c = frx::route_search(G.cells.data(), G.dim, s, g, biggest, D, w, r2);
            CHECK(c.status == frx::ROUTE_CAP_RAW && c.levels == D && r2.empty(), "cap_raw one short: status %d", c.status);
        }
    }
}

void workspace() {
    const int dim[3] = {23, 3, 1};
    const frx::RouteWork w = frx::route_work(dim, 3, 5, 7, 2);
    CHECK(w.verdict == frx::ROUTE_WORK_FITS && w.cells == 69 && w.label_words == 18, "69 cells");
    CHECK(w.slot_off == 0 && w.npts_off == 144 && w.list_off == 160 && w.label_off == 368 && w.bytes == ((w.label_off + 4 * 18 * 3 + 7) & ~(size_t)7), "layout");
    CHECK(w.npts_off % 8 == 0 && w.list_off % 8 == 0 && w.label_off % 8 == 0 && w.bytes % 8 == 0, "alignment");
    const int none[3] = {4, 0, 4}, huge[3] = {1 << 16, 1 << 16, 1}, big[3] = {1 << 15, 1 << 15, 1};
    CHECK(frx::route_work(none, 1, 1, 1, 1).verdict == frx::ROUTE_WORK_INVALID && frx::route_work(huge, 1, 1, 1, 1).verdict == frx::ROUTE_WORK_INVALID, "dims");
    CHECK(frx::route_work(dim, 0, 1, 1, 1).verdict == frx::ROUTE_WORK_INVALID && frx::route_work(dim, 1, 1, 1, 0).verdict == frx::ROUTE_WORK_INVALID, "counts");
    CHECK(frx::route_work(big, 0x7fffffffLL, 0x7fffffffLL, 1, 0x7fffffffLL).verdict == frx::ROUTE_WORK_CAPACITY, "too large");
    const int n3[3] = {5, 4, 1};
    CHECK(frx::route_points(3, n3) == 8 && frx::route_fits(10, 8, 1, 20) && !frx::route_fits(10, 8, 1, 19), "splice bookkeeping");
}

// The rule of a leg's end (route_end_cell): where floatToInt's conversion is defined (a rounded quotient that an int holds) the verdict and the cell are
// floatToInt's; far beyond the map, infinite and not a number are outside, without a conversion the sanitizer could object to.
void ends() {
    const double origin[3] = {-1.2, -2.0, 0.5}, res = 0.1;
    const int dim[3] = {24, 40, 6};
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const double inside[3] = {0.03, 0.41, 0.77};
    int c[3] = {-9, -9, -9};
    CHECK(frx::route_end_cell(origin, res, dim, inside, c) && c[0] == 12 && c[1] == 24 && c[2] == 2, "inside: %d %d %d", c[0], c[1], c[2]);
    std::mt19937 rng(7u);
    std::uniform_real_distribution<double> u(-1.0, 1.0);
    for (int t = 0; t < 20000; t++) {                                             // around the map and a little beyond every face: the defined conversions
        double p[3];
        int want[3];
        bool in = true;
        for (int i = 0; i < 3; i++) {
            p[i] = origin[i] + res * dim[i] * (0.5 + 0.6 * u(rng));
            if (t % 7 == 0) p[i] = origin[i] + res * (double)(int)(rng() % (unsigned)(dim[i] + 3)) - res;   // on cell faces, one cell out included
            want[i] = (int)std::round((p[i] - origin[i]) / res - 0.5);
            in = in && want[i] >= 0 && want[i] < dim[i];
        }
        int got[3] = {-9, -9, -9};
        const bool ok = frx::route_end_cell(origin, res, dim, p, got);
        CHECK(ok == in, "verdict at %.17g %.17g %.17g", p[0], p[1], p[2]);
        if (ok && in) CHECK(got[0] == want[0] && got[1] == want[1] && got[2] == want[2], "cell at %.17g %.17g %.17g", p[0], p[1], p[2]);
        if (!ok) CHECK(got[0] == -9 && got[1] == -9 && got[2] == -9, "an end outside leaves the cell alone");
    }
    const double far[] = {1e6, -1e6, 3e9, -3e9, 1e19, -1e19, 1e300, -1e300, inf, -inf, nan, -nan};
    for (const double v : far)
        for (int axis = 0; axis < 3; axis++) {
            double p[3] = {inside[0], inside[1], inside[2]};
            p[axis] = v;
            int got[3] = {-9, -9, -9};
            CHECK(!frx::route_end_cell(origin, res, dim, p, got) && got[0] == -9 && got[1] == -9 && got[2] == -9, "%g on axis %d is outside", v, axis);
        }
    // one cell beyond dim - 1 on x, where x + dim[0] * y would still index the array
    const double wrap[3] = {origin[0] + res * (dim[0] + 0.5), origin[1] + res * 3.5, origin[2] + res * 1.5};
    CHECK(!frx::route_end_cell(origin, res, dim, wrap, c), "beyond the last cell of a row");
    // a quarter cell beyond either outer face rounds to -1 and to dim (outside); just inside the low face the quotient rounds to -0.0, which is cell 0
    const double lo[3] = {origin[0] - 0.25 * res, inside[1], inside[2]}, hi[3] = {origin[0] + res * (dim[0] + 0.25), inside[1], inside[2]};
    const double lo_in[3] = {origin[0] + 1e-9, inside[1], inside[2]}, hi_in[3] = {origin[0] + res * (dim[0] - 0.25), inside[1], inside[2]};
    CHECK(!frx::route_end_cell(origin, res, dim, lo, c) && !frx::route_end_cell(origin, res, dim, hi, c), "beyond the outer faces");
    CHECK(frx::route_end_cell(origin, res, dim, lo_in, c) && c[0] == 0, "just inside the low face: %d", c[0]);
    CHECK(frx::route_end_cell(origin, res, dim, hi_in, c) && c[0] == dim[0] - 1, "just inside the high face: %d", c[0]);
}

} // namespace

int main() {
    std::mt19937 rng(20240917u);
    frx::RouteScratch w;
    for (int m = 0; m < 1500; m++) one_map(rng, w);
    workspace();
    ends();
    if (failures) { std::printf("route_san: %d checks FAILED\n", failures); return 1; }
    std::printf("route_san: ok\n");
    return 0;
}
