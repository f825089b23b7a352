// Whole safe-flight corridors on the device for a BATCH of paths: the greedy chain of MavGlobalPlanner::plan (MinCoPlan_CPU.cpp:44-83, host form
// frx_corridor_generate in frx_geometry.cpp), one 256-thread workgroup per path.
//
// A chain cannot be batched over its segments - cell m+1 starts at 4/5 of the span the path stays inside cell m, known only once cell m exists - but independent
// paths can, and every step of one chain is a scan: over path points (how far is path[i] visible, how far does the path stay inside the cell) or over the cloud
// (the cell itself, dilate_cell of frx_corridor_kernels.hpp).  Per step:
//   a. segment end k: the first k > i with blocked(P_i, P_k) || |P_i - P_k| >= max_seg, minus one - one lane per k over windows of 256 path points, the first
//      stop by a wave and workgroup minimum; further windows only when a window holds no stop.  The sight line is walked only by lanes the length test let pass.
//   b. the sight line is VoxelMap::blocked (frx_search.cpp) on a device copy of the map's cells.  A cell index is a ROUNDED quotient: one fused multiply-add in
//      pt = a + step * n or in the cell rule flips a sample that lies on a cell border, so map_blocked is compiled with contraction off and keeps the host's order.
//   c. the cell: dilate_cell with offset 0; its records go to the path's slot and stay in LDS beside the candidate buffer.
//   d. exit index j: the first j >= k whose point lies outside a tangent or box plane by more than 1e-10, minus one (windows of 256 path points, records from LDS).
//   e. ceiling and floor appended, i = max(i + 1, (i + 4 j) / 5), until j reaches the last point.
// Every decision (k, j, the record count, the status) is made from values that went through LDS, so all lanes take the same branches and every barrier is
// reached by the whole workgroup.  No atomics, no traffic between workgroups: a path's output depends on that path, the cloud and the map alone.
#pragma once
#include <hip/hip_runtime.h>

#include "frx_corridor_kernels.hpp"

namespace frx {

struct DevVoxelMap {
    double origin[3], res;
    int dim[3];
    const signed char *cells;    // device pointer, x fastest; null: nothing blocks
};

// VoxelMap::blocked (frx_search.cpp; rayTrace + isBlocked, map_util.h:395-425) - same operations in the same order, none fused
__device__ inline bool map_blocked(const DevVoxelMap &m, cg::V3 a, cg::V3 b) {
#pragma clang fp contract(off)
    const double dx = b.x - a.x, dy = b.y - a.y, dz = b.z - a.z;
    const double fx = fabs(dx / m.res), fy = fabs(dy / m.res), fz = fabs(dz / m.res);
    const double fyz = fy < fz ? fz : fy, dmax = fx < fyz ? fyz : fx;             // std::max(fx, std::max(fy, fz))
    const int max_diff = (int)(dmax / 0.8);
    const double s = 1.0 / max_diff;
    const double sx = dx * s, sy = dy * s, sz = dz * s;
    int px = -1, py = -1, pz = -1;
    for (int n = 1; n < max_diff; n++) {
        const double qx = a.x + sx * n, qy = a.y + sy * n, qz = a.z + sz * n;
        const int cx = (int)round((qx - m.origin[0]) / m.res - 0.5), cy = (int)round((qy - m.origin[1]) / m.res - 0.5), cz = (int)round((qz - m.origin[2]) / m.res - 0.5);
        if (cx < 0 || cx >= m.dim[0] || cy < 0 || cy >= m.dim[1] || cz < 0 || cz >= m.dim[2]) break;
        if (cx != px || cy != py || cz != pz)
            if (m.cells[(size_t)cx + (size_t)m.dim[0] * cy + (size_t)m.dim[0] * m.dim[1] * cz] >= 100) return true;
        px = cx; py = cy; pz = cz;
    }
    return false;
}

// tests (frx_debug_map_blocked_device): map_blocked on pairs, one lane per pair
__global__ __launch_bounds__(256) void k_map_blocked_pairs(DevVoxelMap m, int n, const double *a, const double *b, int *out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = map_blocked(m, cg::V3{a[3 * i], a[3 * i + 1], a[3 * i + 2]}, cg::V3{b[3 * i], b[3 * i + 1], b[3 * i + 2]}) ? 1 : 0;
}

enum { CHAIN_OK = 0, CHAIN_BOX_POINTS = 1, CHAIN_PLANES = 2, CHAIN_POLYS = 3 };

struct ChainArgs {
    const int *path_off;         // [n_paths + 1] first point of every path
    const double *path;          // [path_off[n_paths]][3]
    const double *obs;           // [n_obs][3]
    DevVoxelMap map;
    double bbox[3], map_height, max_seg;
    int n_paths, n_obs, cap_polys, cap_planes, pcap;
    double *h_slot;              // [n_paths][cap_polys][cap_planes][6]
    int *cell_planes;            // [n_paths][cap_polys]
    int *n_polys, *status;       // [n_paths]; a path with a non-zero status has n_polys 0
};

// block-wide minimum of v (every lane gets it); wred: 4 ints of LDS
__device__ __forceinline__ int block_min(int v, int *wred) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const int w = __shfl_xor(v, o, 64); v = w < v ? w : v; }
    if ((threadIdx.x & 63) == 0) wred[threadIdx.x >> 6] = v;
    __syncthreads();
    int r = wred[0];
#pragma unroll
    for (int w = 1; w < 4; w++) r = wred[w] < r ? wred[w] : r;
    __syncthreads();
    return r;
}

// the decisions of the chain compare against max_seg and 1e-10 exactly as the host does (frx_geometry.cpp is built without contraction)
__device__ __forceinline__ double chain_dist(cg::V3 a, cg::V3 b) {
#pragma clang fp contract(off)
    const double x = a.x - b.x, y = a.y - b.y, z = a.z - b.z;
    return sqrt(x * x + y * y + z * z);
}
__device__ __forceinline__ bool chain_outside(const double *pl, int np, cg::V3 q) {
#pragma clang fp contract(off)
    bool out = false;
    for (int k = 0; k < np; k++) out = out || (pl[6 * k] * (q.x - pl[6 * k + 3]) + pl[6 * k + 1] * (q.y - pl[6 * k + 4]) + pl[6 * k + 2] * (q.z - pl[6 * k + 5]) > kDecompEpsDev);
    return out;
}

// LDS: the cell's region (dilate_lds_bytes(pcap), rounded up to 8 bytes) | planes[cap_planes][6] doubles | 4 ints
__global__ __launch_bounds__(256) void k_corridor_chain(ChainArgs a) {
    using namespace cg;
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int pth = blockIdx.x, t = threadIdx.x;
    const size_t cell_doubles = (size_t)3 * a.pcap + 32 + 36 + 16 + ((size_t)2 * a.pcap + 257 + 3 + 1) / 2;
    double *planes = sm + cell_doubles;
    int *wred = (int *)(planes + (size_t)6 * a.cap_planes);
    const int p0 = a.path_off[pth], n = a.path_off[pth + 1] - p0;
    const double *path = a.path + (size_t)3 * p0;
    auto P = [&](int i) { return V3{path[3 * i], path[3 * i + 1], path[3 * i + 2]}; };
    const V3 bbox{a.bbox[0], a.bbox[1], a.bbox[2]};
    const int none = 0x7fffffff;
    int m = 0, status = CHAIN_OK;
    for (int i = 0; i < n - 1;) {
        // ---- a. how far path[i] sees and reaches ----
        const V3 pi = P(i);
        int k = n;
        for (int k0 = i + 1; k0 < n; k0 += 256) {
            const int kk = k0 + t;
            bool stop = false;
            if (kk < n) {
                const V3 pk = P(kk);
                stop = chain_dist(pi, pk) >= a.max_seg;
                if (!stop && a.map.cells) stop = map_blocked(a.map, pi, pk);
            }
            const int first = block_min(stop ? kk : none, wred);
            if (first != none) { k = first - 1; break; }
        }
        if (k < i + 1) k = i + 1;
        if (k >= n) k = n - 1;
        // ---- c. the cell ----
        if (m >= a.cap_polys) { status = CHAIN_POLYS; break; }
        double *out = a.h_slot + ((size_t)pth * a.cap_polys + m) * a.cap_planes * 6;
        M3 C; V3 d;
        int np = dilate_cell(pi, P(k), bbox, 0.0, a.obs, a.n_obs, a.pcap, a.cap_planes - 2, sm, out, planes, C, d);
        if (np < 0) { status = np == -1 ? CHAIN_BOX_POINTS : CHAIN_PLANES; break; }
        __syncthreads();                                              // the records are in LDS for every lane
        // ---- d. how far the path stays inside it (before floor and ceiling, as the reference tests) ----
        int j = n;
        for (int j0 = k; j0 < n; j0 += 256) {
            const int jj = j0 + t;
            const bool outside = jj < n && chain_outside(planes, np, P(jj));
            const int first = block_min(outside ? jj : none, wred);
            if (first != none) { j = first; break; }
        }
        j--;
        // ---- e. ceiling, floor, advance (MinCoPlan_CPU.cpp:85-91, :77-82) ----
        if (t < 12) out[6 * np + t] = t == 2 ? 1.0 : t == 5 ? a.map_height : t == 8 ? -1.0 : 0.0;      // (0,0,1 | 0,0,map_height), (0,0,-1 | 0,0,0)
        if (t == 0) a.cell_planes[(size_t)pth * a.cap_polys + m] = np + 2;
        m++;
        if (j >= n - 1) break;
        const int wp = (1 * i + 4 * j) / 5;
        i = wp > i ? wp : i + 1;
        __syncthreads();                                              // every lane has left this cell's LDS before the next one fills it
    }
    if (t == 0) { a.n_polys[pth] = status == CHAIN_OK ? m : 0; a.status[pth] = status; }
}

} // namespace frx
