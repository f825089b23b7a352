// The level search of frx_route_host.hpp confined to a box around a leg's two ends, with a certificate that the box lost nothing.  Plain C++, no
// HIP: frx_search.cpp wraps it (frx_route_plan_levels_window_batch), tests/hostcheck/route_window_main.cpp runs it under the sanitizers against route_search, and
// it is the referee of the device form (frx_route_window_kernel.hpp), which calls route_window as well.
//
// The window of a leg with end cells s, g and a pad of `pad` cells is the box of s and g widened by pad cells on every side and clipped to the map:
//   lo_a = max(0, min(s_a, g_a) - pad),  hi_a = min(dim_a - 1, max(s_a, g_a) + pad).
// A side is CLOSED when it lies on the map's face (lo_a = 0, hi_a = dim_a - 1: the clip took effect, or the pad ended exactly there) - no cell lies beyond it;
// otherwise it is OPEN and lies exactly pad cells from the box of s, g.  A window without an open side is the whole map.
// With M = |s - g|_1: a path from s to g that leaves the window through an open side visits a cell pad + 1 beyond the box of s, g on some axis, so it holds
// at least M + 2 (pad + 1) steps.  limit = M + 2 pad.  When the level search confined to the window labels the start at a level D <= limit, no shortest path of
// the whole map leaves the window; every cell on any shortest path then has the same level inside the window as on the whole map, the descent sees the same
// candidates, and the raw path, `levels` and everything the tail makes of them are the whole-map search's, bit for bit.  When D > limit inside an open window, or
// the levels run dry there, nothing is known: the leg says so (ROUTE_WINDOW_OPEN) and returns no path.
// Labels are indexed inside the window, (x - lo_x) + size_x ((y - lo_y) + size_y (z - lo_z)), one byte a cell as in route_search; the lists and the raw path
// keep whole-map cell ids.  max_level_cells is the largest level built INSIDE THE WINDOW: it may be smaller than the whole-map search's value for the same leg
// (levels of the whole map spread beyond the box), also where the path is identical.
#pragma once
#include "frx_route_host.hpp"

namespace frx {

enum { ROUTE_CAP_WINDOW = 6, ROUTE_WINDOW_OPEN = 7 };                             // a leg's status, beside those of frx_route_host.hpp
enum { ROUTE_PAD_MAX = 1 << 20 };
constexpr long long ROUTE_CAP_WINDOW_MAX = 0x7fffffffLL - 3;                      // window-local indices and the word count times four stay below 2^31

struct RouteWindow {
    int lo[3], size[3];
    long long cells;                                                              // size_x size_y size_z
    bool open;                                                                    // any side open
    int limit;                                                                    // M + 2 pad; -1 for a window without an open side (the whole map)
};

// dim > 0, s and g inside the map, pad in [0, ROUTE_PAD_MAX]
FRX_ROUTE_HD inline RouteWindow route_window(const int *dim, const int *s, const int *g, int pad) {
    RouteWindow w;
    long long m = 0;
    w.cells = 1;
    w.open = false;
    for (int i = 0; i < 3; i++) {
        const long long a = s[i] < g[i] ? s[i] : g[i], b = s[i] < g[i] ? g[i] : s[i];
        long long lo = a - pad, hi = b + pad;
        if (lo <= 0) lo = 0; else w.open = true;
        if (hi >= (long long)dim[i] - 1) hi = (long long)dim[i] - 1; else w.open = true;
        w.lo[i] = (int)lo;
        w.size[i] = (int)(hi - lo + 1);
        w.cells *= hi - lo + 1;
        m += b - a;
    }
    const long long limit = m + 2LL * pad;                                        // a limit no int holds never binds: a window has fewer than 2^31 levels
    w.limit = w.open ? (int)(limit < 0x7fffffffLL ? limit : 0x7fffffffLL) : -1;
    return w;
}

// the row of a leg in leg_window: lo xyz, size xyz, limit, 0
FRX_ROUTE_HD inline void route_window_row(const RouteWindow &w, int *row) {
    for (int i = 0; i < 3; i++) { row[i] = w.lo[i]; row[3 + i] = w.size[i]; }
    row[6] = w.limit;
    row[7] = 0;
}

// route_search inside the leg's window.  The verdicts, in the device's order: more cells than cap_window (ROUTE_CAP_WINDOW, before a label is touched: levels
// -1, max_level_cells 0); a level larger than cap_level; the start labelled; an empty level (ROUTE_NO_PATH in a window without an open side, ROUTE_WINDOW_OPEN
// otherwise); `limit` levels built in an open window without labelling the start (ROUTE_WINDOW_OPEN: no leg builds more than limit levels); cap_raw as in
// route_search.  cap_window, cap_level, cap_raw < 1: no limit.  *win_out, when given, receives the window.
inline RouteSearchOut route_search_window(const signed char *cells, const int *dim, const int *s, const int *g, int pad, long long cap_window, int cap_level,
                                          int cap_raw, RouteScratch &w, std::vector<int> &raw, RouteWindow *win_out = nullptr) {
    const int nx = dim[0], ny = dim[1];
    const long long layer = (long long)nx * ny;
    const RouteWindow win = route_window(dim, s, g, pad);
    if (win_out) *win_out = win;
    raw.clear();
    RouteSearchOut o;
    if (cap_window >= 1 && win.cells > cap_window) { o.status = ROUTE_CAP_WINDOW; return o; }
    if (w.label.size() < (size_t)win.cells) w.label.assign((size_t)win.cells, 0);  // all zero between legs: a leg clears what it touched
    const int lx = win.lo[0], ly = win.lo[1], lz = win.lo[2], sx = win.size[0], sy = win.size[1], sz = win.size[2];
    const auto local = [&](int x, int y, int z) { return (size_t)(x - lx) + (size_t)sx * ((size_t)(y - ly) + (size_t)sy * (size_t)(z - lz)); };
    const int sid = (int)(s[0] + (long long)nx * s[1] + layer * s[2]), gid = (int)(g[0] + (long long)nx * g[1] + layer * g[2]);
    w.cur.assign(1, gid);
    w.touched.assign(1, gid);
    w.label[local(g[0], g[1], g[2])] = 1;
    o.max_level_cells = 1;
    int level = 0;
    bool found = sid == gid;
    while (!found) {
        w.next.clear();
        const unsigned char mark = (unsigned char)(1 + (level + 1) % 3);
        for (const int c : w.cur) {
            const int x = c % nx, y = (int)((c / nx) % ny), z = (int)(c / layer);
            for (int k = 0; k < 6; k++) {
                const int X = x + ROUTE_STEP[k][0], Y = y + ROUTE_STEP[k][1], Z = z + ROUTE_STEP[k][2];
                if (X < lx || X >= lx + sx || Y < ly || Y >= ly + sy || Z < lz || Z >= lz + sz) continue;   // outside the window, the map's faces included
                const int n = (int)(X + (long long)nx * Y + layer * Z);
                const size_t ln = local(X, Y, Z);
                if (cells[n] > 0 || w.label[ln]) continue;
                w.label[ln] = mark;
                w.next.push_back(n);
                if (n == sid) found = true;
            }
        }
        w.touched.insert(w.touched.end(), w.next.begin(), w.next.end());
        if ((int)w.next.size() > o.max_level_cells) o.max_level_cells = (int)w.next.size();
        if (cap_level >= 1 && (int)w.next.size() > cap_level) { o.status = ROUTE_CAP_LEVEL; break; }
        level++;
        if (found) break;
        if (w.next.empty()) { o.status = win.open ? (int)ROUTE_WINDOW_OPEN : (int)ROUTE_NO_PATH; break; }
        if (win.open && level >= win.limit) { o.status = ROUTE_WINDOW_OPEN; break; }
        w.cur.swap(w.next);
    }
    if (o.status == ROUTE_OK) {
        o.levels = level;
        if (cap_raw >= 1 && level + 1 > cap_raw) o.status = ROUTE_CAP_RAW;
    }
    if (o.status == ROUTE_OK) {
        raw.reserve((size_t)level + 1);
        int x = s[0], y = s[1], z = s[2];
        raw.push_back(sid);
        for (int L = level; L > 0; L--) {
            const unsigned char want = (unsigned char)(1 + (L - 1) % 3);
            int best = -1;
            long long best_d = 0;
            for (int k = 0; k < 6; k++) {
                const int X = x + ROUTE_STEP[k][0], Y = y + ROUTE_STEP[k][1], Z = z + ROUTE_STEP[k][2];
                if (X < lx || X >= lx + sx || Y < ly || Y >= ly + sy || Z < lz || Z >= lz + sz) continue;
                if (w.label[local(X, Y, Z)] != want) continue;
                const long long ax = X - g[0], ay = Y - g[1], az = Z - g[2], d = ax * ax + ay * ay + az * az;
                if (best < 0 || d < best_d) best = k, best_d = d;
            }
            // a labelled cell of level L > 0 was claimed from a cell of level L - 1 inside the window: best >= 0
            x += ROUTE_STEP[best][0], y += ROUTE_STEP[best][1], z += ROUTE_STEP[best][2];
            raw.push_back((int)(x + (long long)nx * y + layer * z));
        }
    }
    for (const int c : w.touched) w.label[local(c % nx, (int)((c / nx) % ny), (int)(c / layer))] = 0;
    return o;
}

// The device form's workspace (frx_route_window_workspace): route_work's regions with the labels of one leg sized by cap_window instead of the map.  Per leg
// 24 cap_pts + 4 + 4 (2 cap_level + cap_raw) + 4 ceil(cap_window / 4) bytes, the regions aligned as in route_work, and its three verdicts.  A function of its
// arguments alone: the map's size does not enter.
inline RouteWork route_window_work(long long n_legs, long long cap_level, long long cap_raw, long long cap_pts, long long cap_window) {
    RouteWork w;
    if (n_legs < 1 || cap_level < 1 || cap_raw < 1 || cap_pts < 1 || cap_window < 1 || cap_window > ROUTE_CAP_WINDOW_MAX) return w;
    w.cells = cap_window;
    w.label_words = route_label_words(cap_window);
    const double per_leg = 24.0 * (double)cap_pts + 4.0 + 4.0 * (2.0 * (double)cap_level + (double)cap_raw) + 4.0 * (double)w.label_words;
    w.verdict = ROUTE_WORK_CAPACITY;
    if (n_legs > 0x7fffffffLL || per_leg * (double)n_legs > 4.0e18) return w;
    const auto up8 = [](size_t b) { return (b + 7) & ~(size_t)7; };
    const size_t L = (size_t)n_legs;
    w.slot_off = 0;
    w.npts_off = up8(w.slot_off + 24 * (size_t)cap_pts * L);
    w.list_off = up8(w.npts_off + 4 * L);
    w.label_off = up8(w.list_off + 4 * (2 * (size_t)cap_level + (size_t)cap_raw) * L);
    w.bytes = up8(w.label_off + 4 * w.label_words * L);
    w.verdict = ROUTE_WORK_FITS;
    return w;
}

} // namespace frx
