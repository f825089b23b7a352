// What the handle-less batch entries (frx_batch.cpp) decide on the host, in plain C++ (no HIP): the rule of a voxel map, the task list of the vertex enumeration
// with the argument rules that walk its CSR, the need of a compaction against its capacity, and the compaction itself.  The entries call these functions and so
// does the host build of tests/hostcheck (tests/test_batch_host_cpu.py).  Refusals go through frx::set_error as everywhere.
// (The functions are static: libfrx.so exports the C ABI, not these.)
#pragma once
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "frx_internal.hpp"

namespace frx {

// A voxel map that a kernel indexes: res > 0, dim > 0 on three axes, cells where the entry reads them through the struct (need_cells), and cell indices that stay
// ints - a layer of dim[0] * dim[1] and the whole grid at most 2^31 - 1 cells.  FRX_OK, or FRX_ERR_INVALID_ARG in the name of `who`.  map is not NULL.
static inline int voxel_map_args(const frx_voxel_map *map, const char *who, bool need_cells) {
    if (!(map->res > 0) || map->dim[0] <= 0 || map->dim[1] <= 0 || map->dim[2] <= 0 || (need_cells && !map->cells))
        return set_error(FRX_ERR_INVALID_ARG, std::string(who) + ": the map needs " + (need_cells ? "cells, " : "") + "res > 0 and dim > 0 on all three axes");
    const long long layer = (long long)map->dim[0] * map->dim[1];
    if (layer > 0x7fffffffLL || layer * map->dim[2] > 0x7fffffffLL) return set_error(FRX_ERR_INVALID_ARG, std::string(who) + ": more than 2^31 - 1 map cells");
    return FRX_OK;
}

// ---- the route batch ----
// The rules every form of the route batch shares: the map (cells included), the count of routes and the four capacities; cap_total holds a two-point
// placeholder for every route.
static inline int route_batch_args(const frx_voxel_map *map, const char *who, int n_routes, int cap_level, int cap_raw, int cap_pts, int cap_total) {
    if (!map) return set_error(FRX_ERR_INVALID_ARG, std::string(who) + ": null map");
    if (int rc = voxel_map_args(map, who, true)) return rc;
    if (n_routes < 1) return set_error(FRX_ERR_INVALID_ARG, std::string(who) + ": n_routes < 1");
    if (cap_level < 1 || cap_raw < 1 || cap_pts < 1) return set_error(FRX_ERR_INVALID_ARG, std::string(who) + ": cap_level, cap_raw and cap_pts must be at least 1");
    if ((long long)cap_total < 2LL * n_routes) return set_error(FRX_ERR_INVALID_ARG, std::string(who) + ": cap_total < 2 n_routes (every route keeps room for its two-point placeholder)");
    return FRX_OK;
}
// The rules the window forms add: a pad in [0, 1 << 20] cells and a cap_window in [1, 2^31 - 4] cells (window-local indices stay ints).
static inline int route_window_args(const char *who, int pad, long long cap_window) {
    if (pad < 0 || pad > (1 << 20)) return set_error(FRX_ERR_INVALID_ARG, std::string(who) + ": pad must lie in [0, 1 << 20]");
    if (cap_window < 1 || cap_window > 0x7fffffffLL - 3) return set_error(FRX_ERR_INVALID_ARG, std::string(who) + ": cap_window must lie in [1, 2^31 - 4]");
    return FRX_OK;
}
// The rules that walk the waypoint offsets of host forms; *n_legs: the legs of all routes.
static inline int route_offset_args(const char *who, int n_routes, const int *pt_off, long long *n_legs) {
    if (pt_off[0] < 0) return set_error(FRX_ERR_INVALID_ARG, std::string(who) + ": pt_off[0] < 0");
    for (int r = 0; r < n_routes; r++) {
        if (pt_off[r + 1] < pt_off[r]) return set_error(FRX_ERR_INVALID_ARG, std::string(who) + ": pt_off is not monotone at route " + std::to_string(r));
        if (pt_off[r + 1] - pt_off[r] < 2) return set_error(FRX_ERR_INVALID_ARG, std::string(who) + ": route " + std::to_string(r) + " has fewer than 2 waypoints");
    }
    *n_legs = (long long)pt_off[n_routes] - pt_off[0] - n_routes;
    return FRX_OK;
}

// ---- the vertex enumeration's tasks ----
// The rules that walk coarse_n [B] and the CSR offsets of its polytopes; *n_poly: their number.
static inline int enum_csr_args(const char *who, int B, const int *coarse_n, const int *h_off, long long *n_poly) {
    long long n = 0;
    for (int b = 0; b < B; b++) {
        if (coarse_n[b] < 1) return set_error(FRX_ERR_INVALID_ARG, std::string(who) + ": coarse_n[" + std::to_string(b) + "] < 1");
        n += coarse_n[b];
    }
    if (2 * n - B > 0x7fffffffLL / 4) return set_error(FRX_ERR_INVALID_ARG, std::string(who) + ": too many polytopes");
    if (h_off[0] < 0) return set_error(FRX_ERR_INVALID_ARG, std::string(who) + ": h_off[0] < 0");
    for (long long m = 0; m < n; m++)
        if (h_off[m + 1] < h_off[m]) return set_error(FRX_ERR_INVALID_ARG, std::string(who) + ": h_off is not monotone at polytope " + std::to_string(m));
    *n_poly = n;
    return FRX_OK;
}
// Four ints {first record, planes, second range's first record, its planes} per task, in the order [cell 0, overlap 0|1, cell 1, ...] per candidate; an overlap's
// two ranges are contiguous in this CSR and named apart all the same.  An empty first range would read as "no task": the task takes the second range as its only
// one, and with both empty it carries the plane count -1.
static inline std::vector<int> enum_tasks(int B, const int *coarse_n, const int *h_off) {
    std::vector<int> tasks;
    int poly = 0;
    for (int b = 0; b < B; b++) {
        for (int i = 0; i < coarse_n[b]; i++) {
            const int hb = h_off[poly + i], K = h_off[poly + i + 1] - hb;
            tasks.insert(tasks.end(), {hb, K, 0, 0});
            if (i + 1 < coarse_n[b]) tasks.insert(tasks.end(), {hb, K, h_off[poly + i + 1], h_off[poly + i + 2] - h_off[poly + i + 1]});
        }
        poly += coarse_n[b];
    }
    for (size_t t = 0; t < tasks.size(); t += 4)
        if (tasks[t + 1] == 0) { tasks[t + 1] = tasks[t + 3] ? tasks[t + 3] : -1; tasks[t + 2] = 0; tasks[t + 3] = 0; }
    return tasks;
}

// ---- the compactions ----
// The need of n slots is a long long sum; what *n_rec / *n_vert / v_off report of it is clipped to 2^31 - 1, what is compared with the capacity is not.
static inline long long slots_need(int n, const int *count) { long long need = 0; for (int t = 0; t < n; t++) need += count[t]; return need; }
static inline int clip_count(long long need) { return (int)std::min<long long>(need, 0x7fffffffLL); }
static inline bool need_fits(long long need, int cap, int *reported) { *reported = clip_count(need); return need <= cap; }

// A group of n slots, staged at `widest` rows of W doubles each, of which slot t holds count[t] <= widest: appends the rows in use to the packed records `rec`, of
// which `used` rows are taken, and writes the running offsets off[1 .. n] (off[0] = used is the caller's).  Returns the rows taken after the group.
static inline int pack_slots(int W, int n, const int *count, size_t widest, const double *stage, int used, double *rec, int *off) {
    for (int t = 0; t < n; t++) {
        if (count[t] > 0) std::memcpy(rec + (size_t)W * used, stage + W * widest * t, sizeof(double) * W * (size_t)count[t]);
        used += count[t];
        off[t + 1] = used;
    }
    return used;
}

} // namespace frx
