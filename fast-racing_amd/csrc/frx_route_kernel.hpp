// A batch of routes through the voxel map on the device: the level search of frx_route_host.hpp, plan_leg's tail (frx_search.cpp) and the splice of
// frx_route_plan, for every leg of every route at once.  Four launches:
//   k_route_clear         zeroes the label bytes of all legs
//   k_route_search        one 256-thread workgroup per leg: levels, descent, removeCornerPts twice, removeLinePts, samplePath into the leg's slot
//   k_route_splice_plan   one workgroup: refuses the batch when a route has no waypoint; the points of every route, then - one lane, in route order - its
//                         offset and whether it fits
//   k_route_splice        one workgroup per route: the legs' slots (or the placeholder) into the CSR frx_corridor_generate_batch_device takes
//
// The levels.  A cell's label is one byte, 0 or 1 + (level mod 3), four cells to a 32-bit word across row ends.  A lane that finds a traversable neighbour whose
// byte reads 0 claims it with atomicOr on the word; all claims of one level OR the same value into a byte, so exactly one of them gets the old byte back as 0 and
// appends the cell to the next list through an LDS counter.  A list therefore never holds more than its level, and the pre-check (a relaxed load at workgroup
// scope: it may come from L1) can only err towards one atomic too many (a stale 0).  One barrier per level: the three LDS counters rotate (read, appended,
// zeroed), and the level at which the start was claimed goes through LDS as well, so every lane takes the same exit and every barrier is reached by the whole
// workgroup.
//
// L1.  The label bytes are written by atomics only, which execute at L2; the descent reads them with device-scope atomic loads (__hip_atomic_load, relaxed,
// agent scope), which go to L2 as well - never through a line the compute unit's L1 kept from the pre-checks.
//
// The tail runs in wave 0 alone, without a barrier and without LDS: what the lanes share goes through ballots and shuffles.  The sight line spreads the samples
// n = 1 .. max_diff - 1 of VoxelMap::blocked over the lanes, 64 at a time: blocked = the first sample on a cell >= 100 comes before the first sample outside the
// map (the walk's prev de-duplication cannot change that).  samplePath's d accumulates 0.02; every lane runs the same 64 additions and keeps the one of its
// sample, a sample emits a point when its cell differs from the previous sample's (across chunk and edge ends), and a ballot orders the points.  The vertex
// recurrences (corner removal, removeLinePts) are serial over vertices, each sight line inside them parallel.  The path is kept as cell ids, compacted in place in
// the leg's raw list; every point is the centre of its cell, recomputed by the host's expression.  Built with -ffp-contract=off; the functions that turn
// coordinates into cells carry the pragma as well.
#pragma once
#include <hip/hip_runtime.h>

#include "frx_route_host.hpp"

namespace frx {

enum { ROUTE_THREADS = 256 };

struct RouteArgs {
    double origin[3], res;
    int dim[3];
    const signed char *cells;                 // the map, x fastest
    const int *pt_off;                        // [n_routes + 1]
    const double *pts;                        // waypoints [..][3]
    int n_routes, n_legs, cap_level, cap_raw, cap_pts, cap_total;
    unsigned label_words;                     // words of one leg's labels
    double *slot;                             // [n_legs][cap_pts][3]
    int *npts;                                // [n_legs] points in the slot, 0 for a failed leg
    int *lists;                               // [n_legs][2 cap_level + cap_raw]
    unsigned *labels;                         // [n_legs][label_words]
    int *path_off; double *path;              // [n_routes + 1], [cap_total][3]
    int *route_status, *leg_status, *leg_levels, *leg_max_level;
};

__global__ __launch_bounds__(ROUTE_THREADS) void k_route_clear(unsigned long long *labels, size_t n) {
    for (size_t i = (size_t)blockIdx.x * ROUTE_THREADS + threadIdx.x; i < n; i += (size_t)gridDim.x * ROUTE_THREADS) labels[i] = 0ull;
}

// floatToInt / intToFloat (VoxelMap::to_cell, to_point of frx_search.cpp), one axis
__device__ __forceinline__ int route_cell(const RouteArgs &a, double p, int axis) {
#pragma clang fp contract(off)
    return (int)round((p - a.origin[axis]) / a.res - 0.5);
}
__device__ __forceinline__ double route_centre(const RouteArgs &a, int c, int axis) {
#pragma clang fp contract(off)
    return ((double)c + 0.5) * a.res + a.origin[axis];
}
__device__ __forceinline__ bool route_inside(const RouteArgs &a, int x, int y, int z) {
    return x >= 0 && x < a.dim[0] && y >= 0 && y < a.dim[1] && z >= 0 && z < a.dim[2];
}
__device__ __forceinline__ int route_id(const RouteArgs &a, int x, int y, int z) { return x + a.dim[0] * y + a.dim[0] * a.dim[1] * z; }
// the k-th successor of GridSearch::successors: -x, -y, -z, +z, +y, +x
__device__ __forceinline__ void route_step(int k, int &dx, int &dy, int &dz) {
    dx = k == 0 ? -1 : (k == 5 ? 1 : 0);
    dy = k == 1 ? -1 : (k == 4 ? 1 : 0);
    dz = k == 2 ? -1 : (k == 3 ? 1 : 0);
}

struct RoutePoint { double x, y, z; };
__device__ __forceinline__ RoutePoint route_point_of(const RouteArgs &a, int id) {
    const int nx = a.dim[0], ny = a.dim[1];
    return {route_centre(a, id % nx, 0), route_centre(a, (id / nx) % ny, 1), route_centre(a, id / (nx * ny), 2)};
}
__device__ __forceinline__ double route_norm(RoutePoint p, RoutePoint q) {
#pragma clang fp contract(off)
    const double x = p.x - q.x, y = p.y - q.y, z = p.z - q.z;
    return sqrt(x * x + y * y + z * z);
}

// VoxelMap::blocked with its samples over the 64 lanes of the calling wave; every lane gets the verdict
__device__ inline bool route_blocked(const RouteArgs &m, RoutePoint a, RoutePoint b, int lane) {
#pragma clang fp contract(off)
    const double dx = b.x - a.x, dy = b.y - a.y, dz = b.z - a.z;
    const double fx = fabs(dx / m.res), fy = fabs(dy / m.res), fz = fabs(dz / m.res);
    const double fyz = fy < fz ? fz : fy, dmax = fx < fyz ? fyz : fx;             // std::max(fx, std::max(fy, fz))
    const int max_diff = (int)(dmax / 0.8);
    const double s = 1.0 / max_diff;
    const double sx = dx * s, sy = dy * s, sz = dz * s;
    for (int n0 = 1; n0 < max_diff; n0 += 64) {
        const int n = n0 + lane;
        bool hit = false, out = false;
        if (n < max_diff) {
            const double qx = a.x + sx * n, qy = a.y + sy * n, qz = a.z + sz * n;
            const int cx = route_cell(m, qx, 0), cy = route_cell(m, qy, 1), cz = route_cell(m, qz, 2);
            if (!route_inside(m, cx, cy, cz)) out = true;
            else hit = m.cells[(size_t)cx + (size_t)m.dim[0] * cy + (size_t)m.dim[0] * m.dim[1] * cz] >= 100;
        }
        const unsigned long long bh = __ballot(hit), bo = __ballot(out);
        if (bh | bo) return (bh ? __ffsll((long long)bh) : 65) < (bo ? __ffsll((long long)bo) : 65);
    }
    return false;
}

// lane 0's load of a cell id, handed to every lane of the wave
__device__ __forceinline__ int route_load_id(const int *p, int lane) {
    int v = 0;
    if (lane == 0) v = *p;
    return __shfl(v, 0);
}

// remove_corner_pts over the n cell ids at ids[0 .. n - 1], read in reverse when rev; compacts in place (towards the end it reads from) and returns the new count
__device__ inline int route_corner_pass(const RouteArgs &a, int *ids, int n, bool rev, int lane) {
#pragma clang fp contract(off)
    if (n < 2) return n;
    const double inf = __builtin_huge_val();
    int m = 1;
    RoutePoint prev = route_point_of(a, route_load_id(ids + (rev ? n - 1 : 0), lane));
    int id1 = route_load_id(ids + (rev ? n - 2 : 1), lane);
    RoutePoint p1 = route_point_of(a, id1);
    double cost1 = route_blocked(a, prev, p1, lane) ? inf : route_norm(prev, p1);
    for (int i = 1; i + 1 < n; i++) {
        const int id2 = route_load_id(ids + (rev ? n - 2 - i : i + 1), lane);
        const RoutePoint p2 = route_point_of(a, id2);
        const double cost2 = route_blocked(a, p1, p2, lane) ? inf : route_norm(p1, p2);
        const double cost3 = route_blocked(a, prev, p2, lane) ? inf : route_norm(prev, p2);
        if (cost3 < cost1 + cost2)
            cost1 = cost3;
        else {
            if (lane == 0) ids[rev ? n - 1 - m : m] = id1;
            m++;
            cost1 = route_norm(p1, p2);
            prev = p1;
        }
        id1 = id2;
        p1 = p2;
    }
    if (lane == 0) ids[rev ? n - 1 - m : m] = id1;
    return m + 1;
}

// remove_line_pts over ids[0 .. n - 1], in place; returns the new count
__device__ inline int route_line_pass(const RouteArgs &a, int *ids, int n, int lane) {
#pragma clang fp contract(off)
    if (n < 3) return n;
    int m = 1;
    RoutePoint before = route_point_of(a, route_load_id(ids, lane));
    int idc = route_load_id(ids + 1, lane);
    RoutePoint cur = route_point_of(a, idc);
    for (int i = 1; i + 1 < n; i++) {
        const int idn = route_load_id(ids + i + 1, lane);
        const RoutePoint nxt = route_point_of(a, idn);
        const double ax = nxt.x - cur.x, ay = nxt.y - cur.y, az = nxt.z - cur.z, bx = cur.x - before.x, by = cur.y - before.y, bz = cur.z - before.z;
        const double px = ax - bx, py = ay - by, pz = az - bz;
        if (fabs(px) + fabs(py) + fabs(pz) > 1e-2) {
            if (lane == 0) ids[m] = idc;
            m++;
        }
        before = cur;
        idc = idn;
        cur = nxt;
    }
    if (lane == 0) ids[m] = idc;
    return m + 1;
}

// sample_path over the n vertices ids[0 .. n - 1] into slot (cap points of 3 doubles); returns the points the path has, stored or not
__device__ inline long long route_sample_pass(const RouteArgs &a, const int *ids, int n, double *slot, int cap, int lane) {
#pragma clang fp contract(off)
    int id1 = route_load_id(ids, lane);
    RoutePoint p1 = route_point_of(a, id1);
    if (lane == 0) { slot[0] = p1.x; slot[1] = p1.y; slot[2] = p1.z; }            // cap >= 1
    long long cnt = 1;
    int lx = route_cell(a, p1.x, 0), ly = route_cell(a, p1.y, 1), lz = route_cell(a, p1.z, 2);      // the cell of the sample before
    for (int e = 0; e + 1 < n; e++) {
        const int id2 = route_load_id(ids + e + 1, lane);
        const RoutePoint p2 = route_point_of(a, id2);
        const double l = route_norm(p2, p1);
        double d = 0.0;
        for (bool more = true; more;) {
            double dl = 0.0;
            for (int k = 0; k < 64; k++) {                                       // the reference's accumulation, the same in every lane
                if (lane == k) dl = d;
                d += 0.02;
            }
            const bool act = dl <= l;
            const double w1 = (l - dl) / l, w2 = dl / l;
            const double qx = w1 * p1.x + w2 * p2.x, qy = w1 * p1.y + w2 * p2.y, qz = w1 * p1.z + w2 * p2.z;
            const int cx = route_cell(a, qx, 0), cy = route_cell(a, qy, 1), cz = route_cell(a, qz, 2);
            int bx = __shfl_up(cx, 1), by = __shfl_up(cy, 1), bz = __shfl_up(cz, 1);
            if (lane == 0) { bx = lx; by = ly; bz = lz; }
            const bool emit = act && (cx != bx || cy != by || cz != bz);
            const unsigned long long be = __ballot(emit);
            const long long pos = cnt + __popcll(be & ((1ull << lane) - 1ull));
            if (emit && pos < cap) {
                double *o = slot + 3 * (size_t)pos;
                o[0] = route_centre(a, cx, 0); o[1] = route_centre(a, cy, 1); o[2] = route_centre(a, cz, 2);
            }
            cnt += __popcll(be);
            const int nact = __popcll(__ballot(act));
            if (nact > 0) { lx = __shfl(cx, nact - 1); ly = __shfl(cy, nact - 1); lz = __shfl(cz, nact - 1); }
            more = nact == 64;
        }
        p1 = p2;
    }
    return cnt;
}

__global__ __launch_bounds__(ROUTE_THREADS) void k_route_search(RouteArgs a) {
    __shared__ int s_cnt[3];
    __shared__ int s_found;                                                       // the level whose build claimed the start's cell, -1 before
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
        // route_end_cell decides on the rounded double: an end far outside or not a number never becomes a cell index
        if (!route_end_cell(a.origin, a.res, a.dim, ps, s) || a.cells[sid = route_id(a, s[0], s[1], s[2])] != 0) status = ROUTE_START;
        else if (!route_end_cell(a.origin, a.res, a.dim, ps + 3, g) || a.cells[gid = route_id(a, g[0], g[1], g[2])] != 0) status = ROUTE_GOAL;
    }
    if (status != ROUTE_OK) {                                                     // the same verdict in every lane: nobody reaches a barrier
        if (tid == 0) { a.leg_status[leg] = status; a.leg_levels[leg] = -1; a.leg_max_level[leg] = 0; a.npts[leg] = 0; }
        return;
    }
    unsigned *lab = a.labels + (size_t)leg * a.label_words;
    int *cur = a.lists + (size_t)leg * (2 * (size_t)a.cap_level + a.cap_raw), *nxt = cur + a.cap_level, *raw = cur + 2 * (size_t)a.cap_level;
    const int nx = a.dim[0], ny = a.dim[1], layer = nx * ny;
    if (tid == 0) {
        cur[0] = gid;
        atomicOr(lab + (gid >> 2), 1u << (8 * (gid & 3)));
        s_cnt[0] = 1; s_cnt[1] = 0; s_cnt[2] = 0;
        s_found = -1;
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
                if (!route_inside(a, X, Y, Z)) continue;
                const int n = X + nx * Y + layer * Z;
                if (a.cells[n] > 0) continue;
                unsigned *w = lab + (n >> 2);
                const int sh = 8 * (n & 3);
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
        if (n_next == 0) { status = ROUTE_NO_PATH; break; }
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
                if (route_inside(a, X, Y, Z)) {
                    const int n = X + nx * Y + layer * Z;
                    const unsigned wv = __hip_atomic_load(lab + (n >> 2), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (((wv >> (8 * (n & 3))) & 0xffu) == want) {
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
        // plan_leg's tail: corners forwards, corners backwards, collinear vertices, samples
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

// The points of every route (all lanes), then the offsets in route order (one lane): path_off[r + 1] carries a route's want between the two.
__global__ __launch_bounds__(ROUTE_THREADS) void k_route_splice_plan(RouteArgs a) {
    __shared__ int s_empty;
    const int tid = threadIdx.x, p0 = a.pt_off[0];
    // A route without a waypoint (or offsets that step back) takes a leg slot away from the routes behind it: first = pt_off[r] - p0 - r is no longer monotone
    // and the caller's leg arrays hold fewer slots than legs exist.  The batch is refused whole: every route ROUTE_NO_POINTS with its placeholder, every leg
    // ROUTE_NO_PATH with no points, over whatever k_route_search wrote.
    if (tid == 0) s_empty = 0;
    __syncthreads();
    for (int r = tid; r < a.n_routes; r += ROUTE_THREADS)
        if (a.pt_off[r + 1] - a.pt_off[r] < 1) s_empty = 1;
    __syncthreads();
    const bool refused = s_empty != 0;
    if (refused)
        for (int l = tid; l < a.n_legs; l += ROUTE_THREADS) { a.leg_status[l] = ROUTE_NO_PATH; a.leg_levels[l] = -1; a.leg_max_level[l] = 0; a.npts[l] = 0; }
    for (int r = tid; r < a.n_routes; r += ROUTE_THREADS) {
        const int legs = a.pt_off[r + 1] - a.pt_off[r] - 1, first = a.pt_off[r] - p0 - r;
        int st = ROUTE_WHOLE;
        long long want = 0;
        if (refused || legs < 1 || first < 0 || first + legs > a.n_legs) st = ROUTE_NO_POINTS;
        else {
            for (int l = 0; l < legs; l++) {
                if (a.leg_status[first + l] != ROUTE_OK) st = ROUTE_LEG_FAILED;
                want += a.npts[first + l];
            }
            want -= legs - 1;
        }
        a.route_status[r] = st;
        a.path_off[r + 1] = st == ROUTE_WHOLE ? (int)(want < 0x7fffffffLL ? want : 0x7fffffffLL) : 2;
    }
    __syncthreads();
    if (tid == 0) {
        long long used = 0;
        a.path_off[0] = 0;
        for (int r = 0; r < a.n_routes; r++) {
            long long want = a.path_off[r + 1];
            if (a.route_status[r] == ROUTE_WHOLE && !route_fits(used, want, a.n_routes - 1 - r, a.cap_total)) {
                a.route_status[r] = ROUTE_NO_ROOM;
                want = 2;
            }
            used += want;
            a.path_off[r + 1] = (int)used;
        }
    }
}

__global__ __launch_bounds__(ROUTE_THREADS) void k_route_splice(RouteArgs a) {
    const int r = blockIdx.x, tid = threadIdx.x;
    if (r >= a.n_routes) return;
    const int n_wp = a.pt_off[r + 1] - a.pt_off[r], legs = n_wp - 1, first = a.pt_off[r] - a.pt_off[0] - r;
    double *out = a.path + 3 * (size_t)a.path_off[r];
    if (a.route_status[r] != ROUTE_WHOLE) {
        // the placeholder: the route's first and last waypoint as given (zeros for a route without any)
        if (tid < 6) {
            const int w = tid < 3 ? a.pt_off[r] : a.pt_off[r + 1] - 1;
            out[tid] = n_wp >= 1 ? a.pts[3 * (size_t)w + tid % 3] : 0.0;
        }
        return;
    }
    size_t pos = 0;
    for (int l = 0; l < legs; l++) {
        const int n = a.npts[first + l], take = l + 1 < legs ? n - 1 : n;         // the shared point comes from the leg behind it
        const double *src = a.slot + 3 * (size_t)(first + l) * a.cap_pts;
        for (int i = tid; i < 3 * take; i += ROUTE_THREADS) out[3 * pos + i] = src[i];
        pos += (size_t)take;
    }
}

} // namespace frx
