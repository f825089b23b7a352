// The route batch searched inside certified per-leg windows: k_route_search of frx_route_kernel.hpp with the labels of a leg indexed inside the
// window of frx_route_window_host.hpp, so a leg's label memory is cap_window bytes whatever the map's size, and the flood ends after `limit` levels.  Three
// launches: k_route_search_window, then k_route_splice_plan and k_route_splice as they are (a leg with status 6 or 7 is a failed leg to them).
//
// What is shared with k_route_search: the claim (atomicOr on the word that holds the cell's byte - here the window-local word), the three rotating LDS counters,
// one barrier per level, the descent's agent-scope loads, and the tail's device functions (route_corner_pass, route_line_pass, route_sample_pass), which read
// the map's cells only.  What differs: a neighbour outside the window is skipped like one outside the map; the lists and the raw path keep whole-map ids while
// the labels use (x - lo_x) + size_x ((y - lo_y) + size_y (z - lo_z)); and three more verdicts, each taken from values every lane holds (the window is
// computed by every lane from the same two cells) or that pass through LDS (the level's count, the level that claimed the start): more cells than cap_window,
// an empty level in an open window, `limit` levels without the start.
//
// Clearing.  Each workgroup zeroes the words of its own window - ceil(cells / 4) of them, not the leg's whole cap_window - before its first claim, then
// __threadfence() and a barrier.  No clear launch: the memory touched follows the windows a batch really has (cap_window is sized by the largest), a caller's
// workspace needs no preparation, and a replayed graph clears again because the clear is part of the kernel.  The stores are plain vector stores; the fence
// makes them complete at L2, where the claims execute, before the first atomic, and drops whatever the compute unit's L1 held of the region.
#pragma once
#include "frx_route_kernel.hpp"
#include "frx_route_window_host.hpp"

namespace frx {

struct RouteWindowArgs {
    RouteArgs r;                              // labels: [n_legs][label_words] with label_words = ceil(cap_window / 4)
    int pad;
    long long cap_window;
    int *leg_window;                          // [n_legs][8]
};

__global__ __launch_bounds__(ROUTE_THREADS) void k_route_search_window(RouteWindowArgs wa) {
    __shared__ int s_cnt[3];
    __shared__ int s_found;                                                       // the level whose build claimed the start's cell, -1 before
    const RouteArgs &a = wa.r;
    const int leg = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    if (leg >= a.n_legs) return;
    // the leg's route: the last one whose first leg is not behind this one
    const int p0 = a.pt_off[0];
    int lo = 0, hi = a.n_routes - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.pt_off[mid] - p0 - mid <= leg) lo = mid; else hi = mid - 1;
    }
    const int wp = a.pt_off[lo] + (leg - (a.pt_off[lo] - p0 - lo));
    int status = ROUTE_OK, levels = -1, maxlev = 0;
    int s[3] = {0, 0, 0}, g[3] = {0, 0, 0}, sid = 0, gid = 0;
    if (wp < a.pt_off[lo] || wp + 1 >= a.pt_off[lo + 1]) status = ROUTE_NO_PATH;   // offsets the caller vouched for do not hold this leg
    else {
        const double *ps = a.pts + 3 * (size_t)wp;
        if (!route_end_cell(a.origin, a.res, a.dim, ps, s) || a.cells[sid = route_id(a, s[0], s[1], s[2])] != 0) status = ROUTE_START;
        else if (!route_end_cell(a.origin, a.res, a.dim, ps + 3, g) || a.cells[gid = route_id(a, g[0], g[1], g[2])] != 0) status = ROUTE_GOAL;
    }
    int *row = wa.leg_window + 8 * (size_t)leg;
    if (status != ROUTE_OK) {                                                     // the same verdict in every lane: nobody reaches a barrier
        if (tid < 8) row[tid] = 0;
        if (tid == 0) { a.leg_status[leg] = status; a.leg_levels[leg] = -1; a.leg_max_level[leg] = 0; a.npts[leg] = 0; }
        return;
    }
    const RouteWindow win = route_window(a.dim, s, g, wa.pad);
    if (tid == 0) route_window_row(win, row);
    if (win.cells > wa.cap_window) {                                              // before a label is touched; the same in every lane
        if (tid == 0) { a.leg_status[leg] = ROUTE_CAP_WINDOW; a.leg_levels[leg] = -1; a.leg_max_level[leg] = 0; a.npts[leg] = 0; }
        return;
    }
    const int lx = win.lo[0], ly = win.lo[1], lz = win.lo[2], sx = win.size[0], sy = win.size[1], sz = win.size[2];
    const int hx = lx + sx, hy = ly + sy, hz = lz + sz, slayer = sx * sy;         // cells <= cap_window < 2^31
    unsigned *lab = a.labels + (size_t)leg * a.label_words;
    {
        // this window's words: a head up to a 16-byte boundary, four words a store, a tail
        const unsigned n_words = (unsigned)((win.cells + 3) >> 2);               // <= label_words
        unsigned head = (unsigned)((4u - (unsigned)(((size_t)lab >> 2) & 3u)) & 3u);
        if (head > n_words) head = n_words;
        const unsigned n_vec = (n_words - head) >> 2, tail0 = head + 4u * n_vec;
        if ((unsigned)tid < head) lab[tid] = 0u;
        uint4 *v = (uint4 *)(lab + head);
        for (unsigned i = (unsigned)tid; i < n_vec; i += ROUTE_THREADS) v[i] = make_uint4(0u, 0u, 0u, 0u);
        if (tail0 + (unsigned)tid < n_words) lab[tail0 + tid] = 0u;
    }
    int *cur = a.lists + (size_t)leg * (2 * (size_t)a.cap_level + a.cap_raw), *nxt = cur + a.cap_level, *raw = cur + 2 * (size_t)a.cap_level;
    const int nx = a.dim[0], ny = a.dim[1], layer = nx * ny;
    if (tid == 0) {
        cur[0] = gid;
        s_cnt[0] = 1; s_cnt[1] = 0; s_cnt[2] = 0;
        s_found = -1;
    }
    __threadfence();
    __syncthreads();
    if (tid == 0) {
        const int gl = (g[0] - lx) + sx * (g[1] - ly) + slayer * (g[2] - lz);
        atomicOr(lab + (gl >> 2), 1u << (8 * (gl & 3)));
    }
    __syncthreads();
    maxlev = 1;
    int level = 0;
    bool found = sid == gid;
    while (!found) {
        const int n_cur = s_cnt[level % 3];
        int *cnt = &s_cnt[(level + 1) % 3];
        if (tid == 0) s_cnt[(level + 2) % 3] = 0;                                 // the counter after next: read last before the barrier behind us
        const unsigned mark = 1u + (unsigned)((level + 1) % 3);
        for (int i = tid; i < n_cur; i += ROUTE_THREADS) {
            const int c = cur[i], x = c % nx, y = (c / nx) % ny, z = c / layer;
#pragma unroll
            for (int k = 0; k < 6; k++) {
                int dx, dy, dz;
                route_step(k, dx, dy, dz);
                const int X = x + dx, Y = y + dy, Z = z + dz;
                if (X < lx || X >= hx || Y < ly || Y >= hy || Z < lz || Z >= hz) continue;   // outside the window, the map's faces included
                const int n = X + nx * Y + layer * Z;
                if (a.cells[n] > 0) continue;
                const int ln = (X - lx) + sx * (Y - ly) + slayer * (Z - lz);
                unsigned *w = lab + (ln >> 2);
                const int sh = 8 * (ln & 3);
                if ((__hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) >> sh) & 0xffu) continue;   // a stale 0 costs one atomic, the atomic decides
                const unsigned old = atomicOr(w, mark << sh);
                if ((old >> sh) & 0xffu) continue;
                const int at = atomicAdd(cnt, 1);
                if (at < a.cap_level) nxt[at] = n;
                if (n == sid) s_found = level + 1;
            }
        }
        __syncthreads();
        const int n_next = *cnt;
        if (n_next > maxlev) maxlev = n_next;
        if (n_next > a.cap_level) { status = ROUTE_CAP_LEVEL; break; }
        level++;
        if (s_found == level) { found = true; break; }
        if (n_next == 0) { status = win.open ? (int)ROUTE_WINDOW_OPEN : (int)ROUTE_NO_PATH; break; }
        if (win.open && level >= win.limit) { status = ROUTE_WINDOW_OPEN; break; }   // limit levels built, the start not among them: nothing is known
        int *t = cur; cur = nxt; nxt = t;
    }
    if (status == ROUTE_OK) {
        levels = level;
        if (levels + 1 > a.cap_raw) status = ROUTE_CAP_RAW;
    }
    if (tid >= 64) return;                                                        // no barrier from here on: wave 0 walks the path

    long long cnt_pts = 0;
    if (status == ROUTE_OK) {
        // the descent: lanes 0 .. 5 read one neighbour's label each, every lane picks among the six in the successor order
        int x = s[0], y = s[1], z = s[2];
        if (lane == 0) raw[0] = sid;
        for (int L = levels; L > 0; L--) {
            const unsigned want = 1u + (unsigned)((L - 1) % 3);
            int ok = 0;
            long long d = 0;
            if (lane < 6) {
                int dx, dy, dz;
                route_step(lane, dx, dy, dz);
                const int X = x + dx, Y = y + dy, Z = z + dz;
                if (X >= lx && X < hx && Y >= ly && Y < hy && Z >= lz && Z < hz) {
                    const int ln = (X - lx) + sx * (Y - ly) + slayer * (Z - lz);
                    const unsigned wv = __hip_atomic_load(lab + (ln >> 2), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (((wv >> (8 * (ln & 3))) & 0xffu) == want) {
                        const long long ax = X - g[0], ay = Y - g[1], az = Z - g[2];
                        ok = 1;
                        d = ax * ax + ay * ay + az * az;
                    }
                }
            }
            int best = -1;
            long long best_d = 0;
#pragma unroll
            for (int k = 0; k < 6; k++) {
                const int okk = __shfl(ok, k);
                const long long dk = __shfl(d, k);
                if (okk && (best < 0 || dk < best_d)) { best = k; best_d = dk; }
            }
            if (best < 0) { status = ROUTE_NO_PATH; break; }                      // cannot happen: a cell of level L was claimed from level L - 1
            int dx, dy, dz;
            route_step(best, dx, dy, dz);
            x += dx; y += dy; z += dz;
            if (lane == 0) raw[levels - L + 1] = x + nx * y + layer * z;
        }
    }
    if (status == ROUTE_OK) {
        // plan_leg's tail, the passes of frx_route_kernel.hpp on whole-map ids
        int n = levels + 1;
        int m = route_corner_pass(a, raw, n, false, lane);                         // raw[0 .. m)
        const int m2 = route_corner_pass(a, raw, m, true, lane);                   // raw[m - m2 .. m)
        int *path = raw + (m - m2);
        n = route_line_pass(a, path, m2, lane);
        cnt_pts = route_sample_pass(a, path, n, a.slot + 3 * (size_t)leg * a.cap_pts, a.cap_pts, lane);
        if (cnt_pts > a.cap_pts) status = ROUTE_CAP_PTS;
    }
    if (lane == 0) {
        a.leg_status[leg] = status;
        a.leg_levels[leg] = levels;
        a.leg_max_level[leg] = maxlev;
        a.npts[leg] = status == ROUTE_OK ? (int)cnt_pts : 0;
    }
}

} // namespace frx
