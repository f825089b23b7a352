// The level search inside per-leg windows (csrc/frx_route_window_host.hpp) under the address and undefined-behaviour sanitizers, against route_search of
// csrc/frx_route_host.hpp on random small maps.  The rule under test: the windowed status is 0 exactly when the whole-map search finds a path of at most
// M + 2 pad steps or the window is the whole map (and the whole-map search finds one); in every such case the raw path is identical cell for cell and so is
// `levels`; a leg without a certificate reads 7 in an open window and -1 in a whole-map one; no leg builds more than `limit` levels; cap_window is exact.
// route_window itself at pads 0 and 1 << 20 and on ends in the map's corners, and the workspace against its closed form.  Host code only: a program of its
// own, never loaded into Python and never run on a GPU machine (make -C fast-racing_amd/csrc route_window_san && tests/hostcheck/route_window_san).
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../fast-racing_amd/csrc/frx_route_window_host.hpp"

namespace {

int failures = 0;
#define CHECK(cond, ...)                                                  \
    do {                                                                  \
        if (!(cond)) {                                                    \
            if (failures++ < 20) { std::printf("FAILED %s:%d %s  ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
        }                                                                 \
    } while (0)

int n_whole = 0, n_certified = 0, n_open_refused = 0, n_legs = 0;

// the window by its definition, side by side
void window_by_definition(const int *dim, const int *s, const int *g, int pad, const frx::RouteWindow &w) {
    long long cells = 1, m = 0;
    bool open = false;
    for (int i = 0; i < 3; i++) {
        const long long a = std::min(s[i], g[i]), b = std::max(s[i], g[i]);
        const long long lo = std::max(0LL, a - pad), hi = std::min((long long)dim[i] - 1, b + pad);
        CHECK(w.lo[i] == lo && w.size[i] == hi - lo + 1, "axis %d: lo %d size %d", i, w.lo[i], w.size[i]);
        CHECK(lo <= a && b <= hi && lo >= 0 && hi < dim[i], "axis %d: the ends lie inside the window and the window inside the map", i);
        if (lo > 0) { open = true; CHECK(a - lo == pad, "an open low side lies pad cells from the ends' box"); }
        if (hi < dim[i] - 1) { open = true; CHECK(hi - b == pad, "an open high side lies pad cells from the ends' box"); }
        cells *= hi - lo + 1;
        m += b - a;
    }
    CHECK(w.cells == cells && w.open == open, "cells %lld open %d", w.cells, (int)w.open);
    CHECK(w.limit == (open ? m + 2LL * pad : -1), "limit %d", w.limit);
    if (!open) CHECK(w.lo[0] == 0 && w.lo[1] == 0 && w.lo[2] == 0 && w.size[0] == dim[0] && w.size[1] == dim[1] && w.size[2] == dim[2], "no open side: the whole map");
}

void one_map(std::mt19937 &rng, frx::RouteScratch &w) {
    int dim[3] = {3 + (int)(rng() % 12), 3 + (int)(rng() % 12), 1 + (int)(rng() % 5)};
    const int n = dim[0] * dim[1] * dim[2];
    std::vector<signed char> cells(n);
    const unsigned occ = 10 + rng() % 26;
    for (auto &c : cells) { const unsigned r = rng() % 100; c = r < occ ? 100 : (r < occ + 3 ? -1 : 0); }
    std::vector<int> raw, wraw;
    for (int trial = 0; trial < 4; trial++) {
        int s[3], g[3];
        for (int i = 0; i < 3; i++) { s[i] = (int)(rng() % dim[i]); g[i] = (int)(rng() % dim[i]); }
        const auto id = [&](const int *c) { return c[0] + dim[0] * c[1] + dim[0] * dim[1] * c[2]; };
        if (cells[id(s)] > 0 || cells[id(g)] > 0) continue;                       // the callers check the ends
        const int pad = (int)(rng() % 5);
        n_legs++;
        const frx::RouteSearchOut full = frx::route_search(cells.data(), dim, s, g, 0, 0, w, raw);
        frx::RouteWindow win;
        const frx::RouteSearchOut o = frx::route_search_window(cells.data(), dim, s, g, pad, 0, 0, 0, w, wraw, &win);
        for (const unsigned char b : w.label) CHECK(b == 0, "labels not cleared");
        window_by_definition(dim, s, g, pad, win);
        const bool path = full.status == frx::ROUTE_OK;
        const bool expect_ok = path && (!win.open || full.levels <= win.limit);
        CHECK((o.status == frx::ROUTE_OK) == expect_ok, "status %d; whole map %d levels %d, limit %d", o.status, full.status, full.levels, win.limit);
        if (o.status == frx::ROUTE_OK) {
            CHECK(o.levels == full.levels && wraw == raw, "a certified leg is the whole-map leg: levels %d against %d", o.levels, full.levels);
            CHECK(o.max_level_cells <= full.max_level_cells && o.max_level_cells >= 1, "largest level %d against %d", o.max_level_cells, full.max_level_cells);
            if (win.open) n_certified++;
        } else {
            CHECK(o.status == (win.open ? (int)frx::ROUTE_WINDOW_OPEN : (int)frx::ROUTE_NO_PATH) && o.levels == -1 && wraw.empty(), "status %d open %d", o.status, (int)win.open);
            if (win.open) n_open_refused++;
        }
        if (!win.open) {
            n_whole++;
            CHECK(o.status == full.status && o.max_level_cells == full.max_level_cells, "a whole-map window is route_search");
        }
        // the capacities: cap_window exact and before anything else, the others as in route_search
        std::vector<int> r2;
        frx::RouteSearchOut c = frx::route_search_window(cells.data(), dim, s, g, pad, win.cells, 0, 0, w, r2);
        CHECK(c.status == o.status && c.levels == o.levels && c.max_level_cells == o.max_level_cells && r2 == wraw, "cap_window at the window's cells");
        if (win.cells > 1) {
            c = frx::route_search_window(cells.data(), dim, s, g, pad, win.cells - 1, 1, 1, w, r2);
            CHECK(c.status == frx::ROUTE_CAP_WINDOW && c.levels == -1 && c.max_level_cells == 0 && r2.empty(), "cap_window one short: status %d", c.status);
        }
        if (o.status == frx::ROUTE_OK) {
            c = frx::route_search_window(cells.data(), dim, s, g, pad, win.cells, o.max_level_cells, o.levels + 1, w, r2);
            CHECK(c.status == frx::ROUTE_OK && r2 == wraw, "at the exact capacities");
            if (o.max_level_cells > 1) {
                c = frx::route_search_window(cells.data(), dim, s, g, pad, win.cells, o.max_level_cells - 1, o.levels + 1, w, r2);
                CHECK(c.status == frx::ROUTE_CAP_LEVEL && c.levels == -1 && r2.empty(), "cap_level one short: status %d", c.status);
            }
            if (o.levels >= 1) {
                c = frx::route_search_window(cells.data(), dim, s, g, pad, win.cells, o.max_level_cells, o.levels, w, r2);
                CHECK(c.status == frx::ROUTE_CAP_RAW && c.levels == o.levels && r2.empty(), "cap_raw one short: status %d", c.status);
            }
        }
        for (const unsigned char b : w.label) CHECK(b == 0, "labels not cleared after a refused search");
    }
}

void windows() {
    const int dim[3] = {700, 4000, 28};
    const int corners[4][3] = {{0, 0, 0}, {699, 3999, 27}, {0, 3999, 0}, {699, 0, 27}};
    const int pads[] = {0, 1, 20, 1 << 20};
    for (const auto &s : corners)
        for (const auto &g : corners)
            for (const int pad : pads) window_by_definition(dim, s, g, pad, frx::route_window(dim, s, g, pad));
    const int s[3] = {100, 2000, 10}, g[3] = {130, 2100, 12};
    for (const int pad : pads) window_by_definition(dim, s, g, pad, frx::route_window(dim, s, g, pad));
    frx::RouteWindow w = frx::route_window(dim, s, g, 0);
    CHECK(w.open && w.cells == 31LL * 101 * 3 && w.limit == 132, "pad 0: the box of the ends, limit M");
    w = frx::route_window(dim, s, g, 1 << 20);
    CHECK(!w.open && w.cells == 700LL * 4000 * 28 && w.limit == -1, "pad 1 << 20: the whole map");
    w = frx::route_window(dim, s, g, 20);
    CHECK(w.open && w.lo[2] == 0 && w.size[2] == 28 && w.size[0] == 71 && w.size[1] == 141 && w.limit == 172, "pad 20: z closed on both sides");
    w = frx::route_window(dim, corners[0], corners[1], 0);
    CHECK(!w.open && w.limit == -1, "opposite corners at pad 0: every side on a face of the map");
    w = frx::route_window(dim, corners[0], corners[0], 0);
    CHECK(w.open && w.cells == 1 && w.limit == 0, "one cell in a corner: three sides open, limit 0");
    // the largest map the entries take, ends at both ends of it: 64-bit all the way, the limit clipped to an int
    const int line[3] = {0x7fffffff, 1, 1}, a[3] = {0, 0, 0}, b[3] = {0x7ffffffe, 0, 0};
    w = frx::route_window(line, a, b, 1 << 20);
    CHECK(!w.open && w.cells == 0x7fffffffLL && w.limit == -1, "a line of 2^31 - 1 cells");
    const int c[3] = {0x7ffffffd, 0, 0}, d[3] = {(1 << 20) + 1, 0, 0};            // M + 2 pad = 2^31 - 4 + 2^20
    w = frx::route_window(line, d, c, 1 << 20);
    CHECK(w.open && w.limit == 0x7fffffff && w.lo[0] == 1 && w.cells == 0x7ffffffeLL, "a limit beyond an int is clipped: %d", w.limit);
}

void workspace() {
    const frx::RouteWork w = frx::route_window_work(3, 5, 7, 2, 69);
    CHECK(w.verdict == frx::ROUTE_WORK_FITS && w.cells == 69 && w.label_words == 18, "69 cells");
    CHECK(w.slot_off == 0 && w.npts_off == 144 && w.list_off == 160 && w.label_off == 368 && w.bytes == ((w.label_off + 4 * 18 * 3 + 7) & ~(size_t)7), "layout");
    const int dim[3] = {23, 3, 1};
    const frx::RouteWork m = frx::route_work(dim, 3, 5, 7, 2);
    CHECK(m.bytes == w.bytes && m.label_off == w.label_off, "a cap_window of the map's cells is route_work's layout");
    CHECK(frx::route_window_work(0, 1, 1, 1, 1).verdict == frx::ROUTE_WORK_INVALID && frx::route_window_work(1, 0, 1, 1, 1).verdict == frx::ROUTE_WORK_INVALID &&
          frx::route_window_work(1, 1, 0, 1, 1).verdict == frx::ROUTE_WORK_INVALID && frx::route_window_work(1, 1, 1, 0, 1).verdict == frx::ROUTE_WORK_INVALID, "counts");
    CHECK(frx::route_window_work(1, 1, 1, 1, 0).verdict == frx::ROUTE_WORK_INVALID && frx::route_window_work(1, 1, 1, 1, 0x7fffffffLL - 2).verdict == frx::ROUTE_WORK_INVALID &&
          frx::route_window_work(1, 1, 1, 1, 0x7fffffffLL - 3).verdict == frx::ROUTE_WORK_FITS, "cap_window in [1, 2^31 - 4]");
    CHECK(frx::route_window_work(0x7fffffffLL, 0x7fffffffLL, 1, 0x7fffffffLL, 1 << 20).verdict == frx::ROUTE_WORK_CAPACITY, "too large");
}

} // namespace

int main() {
    std::mt19937 rng(20241021u);
    frx::RouteScratch w;
    for (int m = 0; m < 1500; m++) one_map(rng, w);
    windows();
    workspace();
    std::printf("route_window_san: %d legs: %d in a whole-map window, %d certified in an open window, %d refused in an open window\n", n_legs, n_whole, n_certified,
                n_open_refused);
    CHECK(n_whole >= 100 && n_certified >= 500 && n_open_refused >= 100, "the mix of cases");
    if (failures) { std::printf("route_window_san: %d checks FAILED\n", failures); return 1; }
    std::printf("route_window_san: ok\n");
    return 0;
}
