// The canonical level search of a leg on the voxel grid, and the splice of a route's legs, in plain C++.  frx_search.cpp wraps it
// (frx_grid_search_levels, frx_route_plan_levels_batch), tests/hostcheck/route_main.cpp runs it under the sanitizers, and it is the referee of the device form
// (frx_route_kernel.hpp), which builds the same levels with atomics and walks the same descent.
//
// The reference plans with A*, eps = 1, six face neighbours, unit step cost (MinCoPlan_CPU.cpp:13, graph_search.cpp:29-38): the length of its path is the
// breadth-first distance, an integer.  WHICH of the equally short paths it returns depends on the order of its heap operations; this search returns another one
// of the same length, chosen by a rule that needs no order of events:
//   grid      a cell is traversable when it is inside the map and cells <= 0 (the search view, search_cells of frx_search.cpp: unknown cells are crossed)
//   levels    level 0 = the goal's cell; level L + 1 = every traversable, unlabelled face neighbour of a level-L cell.  Levels are built whole; the search
//             stops after the first level that labels the start's cell, or with ROUTE_NO_PATH when a level comes out empty first
//   descent   from the start's cell at level D, step to the face neighbour at level D - 1 whose squared cell distance to the goal (64-bit integers) is
//             smallest, ties in the successor order of GridSearch::successors: -x, -y, -z, +z, +y, +x; repeat down to level 0
//   raw path  start first, D + 1 cells; start and goal in one cell: one cell, D = 0
// The label of a cell is one byte, 0 = unlabelled, else 1 + (level mod 3): face neighbours differ by at most one level, so three values tell the level below
// from the level itself and the level above.  Nothing here is floating point.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

// what the kernels call as well
#if defined(__HIPCC__)
#define FRX_ROUTE_HD __host__ __device__
#else
#define FRX_ROUTE_HD
#endif

namespace frx {

enum { ROUTE_OK = 0, ROUTE_START = 1, ROUTE_GOAL = 2, ROUTE_NO_PATH = -1, ROUTE_CAP_LEVEL = 3, ROUTE_CAP_RAW = 4, ROUTE_CAP_PTS = 5 };   // a leg's status
enum { ROUTE_WHOLE = 0, ROUTE_LEG_FAILED = 1, ROUTE_NO_ROOM = 2, ROUTE_NO_POINTS = 3 };                                                 // a route's status

// the successor order of GridSearch::successors in 3-D
constexpr int ROUTE_STEP[6][3] = {{-1, 0, 0}, {0, -1, 0}, {0, 0, -1}, {0, 0, 1}, {0, 1, 0}, {1, 0, 0}};

// An end of a leg: waypoint -> cell, or outside.  The quotient is the one of floatToInt (VoxelMap::to_cell); the verdict is taken on the rounded double, before
// any conversion to int, so a coordinate far beyond the map, infinite or not a number is outside on the host and on the device alike (the conversion of such
// a double to int is undefined on the host and gives 0, a cell of the map, on the device).  c is written only for an end inside.
FRX_ROUTE_HD inline bool route_end_cell(const double *origin, double res, const int *dim, const double *p, int *c) {
    double q[3];                                                                  // a difference, a quotient, a difference: nothing to contract
    for (int i = 0; i < 3; i++) {
        q[i] = std::round((p[i] - origin[i]) / res - 0.5);
        if (!(q[i] >= 0.0 && q[i] < (double)dim[i])) return false;
    }
    for (int i = 0; i < 3; i++) c[i] = (int)q[i];
    return true;
}

// label bytes of one leg, padded to whole 32-bit words (the device claims a cell with an atomic on the word that holds its byte)
inline size_t route_label_words(long long n_cells) { return (size_t)((n_cells + 3) / 4); }

struct RouteSearchOut {
    int status = ROUTE_OK;
    int levels = -1;             // the start's level D; -1 when the start was not labelled
    int max_level_cells = 0;     // the largest level built, the last one included (level 0 counts: 1)
};

// Scratch of the search, kept between legs: the labels are cleared cell by cell from the lists of what a leg touched.
struct RouteScratch {
    std::vector<unsigned char> label;
    std::vector<int> touched, cur, next;
    void fit(size_t n_cells) { if (label.size() != n_cells) label.assign(n_cells, 0); }
};

// The search alone.  cells: the map's cells or any occupancy array (<= 0 traversable), x fastest; s, g: inside the grid and traversable (the caller has
// checked).  raw: the D + 1 cell ids of the path, start first, filled when status is ROUTE_OK.  cap_level < 1: no limit on a level; cap_raw < 1: none on the path.
inline RouteSearchOut route_search(const signed char *cells, const int *dim, const int *s, const int *g, int cap_level, int cap_raw, RouteScratch &w,
                                   std::vector<int> &raw) {
    const int nx = dim[0], ny = dim[1], nz = dim[2];
    const long long layer = (long long)nx * ny;
    w.fit((size_t)(layer * nz));
    raw.clear();
    RouteSearchOut o;
    const int sid = (int)(s[0] + (long long)nx * s[1] + layer * s[2]), gid = (int)(g[0] + (long long)nx * g[1] + layer * g[2]);
    w.cur.assign(1, gid);
    w.touched.assign(1, gid);
    w.label[gid] = 1;
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
                if (X < 0 || X >= nx || Y < 0 || Y >= ny || Z < 0 || Z >= nz) continue;
                const int n = (int)(X + (long long)nx * Y + layer * Z);
                if (cells[n] > 0 || w.label[n]) continue;
                w.label[n] = mark;
                w.next.push_back(n);
                if (n == sid) found = true;
            }
        }
        w.touched.insert(w.touched.end(), w.next.begin(), w.next.end());
        if ((int)w.next.size() > o.max_level_cells) o.max_level_cells = (int)w.next.size();
        // the verdicts in the device's order: a level too large for its list, the start labelled, an empty level
        if (cap_level >= 1 && (int)w.next.size() > cap_level) { o.status = ROUTE_CAP_LEVEL; break; }
        level++;
        if (found) break;
        if (w.next.empty()) { o.status = ROUTE_NO_PATH; break; }
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
                if (X < 0 || X >= nx || Y < 0 || Y >= ny || Z < 0 || Z >= nz) continue;
                if (w.label[(size_t)(X + (long long)nx * Y + layer * Z)] != want) continue;
                const long long ax = X - g[0], ay = Y - g[1], az = Z - g[2], d = ax * ax + ay * ay + az * az;
                if (best < 0 || d < best_d) best = k, best_d = d;
            }
            // a labelled cell of level L > 0 was claimed from a cell of level L - 1: best >= 0
            x += ROUTE_STEP[best][0], y += ROUTE_STEP[best][1], z += ROUTE_STEP[best][2];
            raw.push_back((int)(x + (long long)nx * y + layer * z));
        }
    }
    for (const int c : w.touched) w.label[c] = 0;
    return o;
}

// The device form's workspace (frx_route_search_workspace): per leg a slot of cap_pts sample points, its point count, two level lists of cap_level cell ids
// and cap_raw raw cells, and one label byte per cell padded to a whole word.  A function of its arguments alone.
enum { ROUTE_WORK_FITS = 0, ROUTE_WORK_INVALID = 1, ROUTE_WORK_CAPACITY = 2 };
struct RouteWork {
    int verdict = ROUTE_WORK_INVALID;
    long long cells = 0;
    size_t label_words = 0;                                   // 32-bit words of one leg's labels
    size_t slot_off = 0, npts_off = 0, list_off = 0, label_off = 0, bytes = 0;   // byte offsets of the four regions, each a multiple of 8
};
inline RouteWork route_work(const int *dim, long long n_legs, long long cap_level, long long cap_raw, long long cap_pts) {
    RouteWork w;
    if (dim[0] <= 0 || dim[1] <= 0 || dim[2] <= 0 || n_legs < 1 || cap_level < 1 || cap_raw < 1 || cap_pts < 1) return w;
    const long long layer = (long long)dim[0] * dim[1];
    if (layer > 0x7fffffffLL || layer * dim[2] > 0x7fffffffLL) return w;
    w.cells = layer * dim[2];
    w.label_words = route_label_words(w.cells);
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

// The splice's bookkeeping for one route, shared by the host batch and restated by k_route_splice_plan: the points of a route whose legs hold n[0 .. legs - 1]
// sample points, the shared point of consecutive legs kept once.
inline long long route_points(int legs, const int *n) {
    long long t = 0;
    for (int l = 0; l < legs; l++) t += n[l];
    return t - (legs - 1);
}

// Does a route of `want` points fit at offset `used` when every one of the `later` routes behind it must still find room for its two-point placeholder?
FRX_ROUTE_HD inline bool route_fits(long long used, long long want, long long later, long long cap_total) { return used + want + 2 * later <= cap_total; }

} // namespace frx
