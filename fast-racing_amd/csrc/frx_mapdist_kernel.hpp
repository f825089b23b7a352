// A batch of trajectories screened against a field over the voxel map's grid (frx_trajectory_map_distance, include/frx.h): per fine piece, the M + 1 samples
// s_j = j (T / M) of the check and the clearance kernels, each one's cell by map_blocked's rule (frx_chain_kernel.hpp) - round((p - origin) / res - 0.5), none of
// it fused: the translation unit is built without contraction - and one look-up of field[cell].  A row:
//   0 the smallest field value over the samples inside the map   1 s_j of that sample   2 its linear cell index   3 the number of samples outside the map
// under the total order (value, j): a value that is not a number first, then the smaller value, then the lower j.  No sample inside: +inf, -1, -1.
//
// Shape: one wave per piece, four pieces per workgroup; lane l takes the samples j = l, l + 64, ... in ascending order, so `<` keeps a lane's lowest j, and the
// lanes are folded with the order by shuffles.  P (M + 1) independent look-ups and nothing else to wait for: the kernel is bound by memory latency, and the
// wave's 64 look-ups in flight are what hides it.  No LDS, no atomics; a row depends on its own piece, the map and the field alone.
#pragma once
#include <hip/hip_runtime.h>

#include "frx_device.hpp"

namespace frx {

static constexpr int MAPDIST_THREADS = 256;

struct MapDistArgs {
    double origin[3], res;
    int dim[3];
    const double *field;                 // [nz][ny][nx]
    const double *T, *C;                 // [P], [P][18]
    int P, M;
    double *rows;                        // [P][4]
};

// (v, j) a before (v, j) b: NaN beats any number, then the smaller value, then the lower j
__device__ __forceinline__ bool mapdist_before(double a, int ja, double b, int jb) {
    const bool na = a != a, nb = b != b;
    if (na || nb) return na && (!nb || ja < jb);
    return a < b || (a == b && ja < jb);
}

__global__ void __launch_bounds__(MAPDIST_THREADS) k_traj_map_distance(MapDistArgs a) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63, piece = blockIdx.x * (MAPDIST_THREADS / 64) + (threadIdx.x >> 6);
    if (piece >= a.P) return;                                             // (whole waves leave: the shuffles below stay among live lanes)
    double c[18];
#pragma unroll
    for (int k = 0; k < 18; k++) c[k] = a.C[(size_t)piece * 18 + k];
    const double step = a.T[piece] / a.M;                                 // the step first, then multiplied, as the check forms it
    double bv = __builtin_huge_val();                                     // identity: +inf with the highest key
    int bj = 0x7fffffff, bc = -1, out = 0;
    for (int j = lane; j <= a.M; j += 64) {
        const double s1 = step * j;
        double p[3];
        poly_eval<0>(c, s1, p);
        const double cx = round((p[0] - a.origin[0]) / a.res - 0.5), cy = round((p[1] - a.origin[1]) / a.res - 0.5), cz = round((p[2] - a.origin[2]) / a.res - 0.5);
        const bool inside = cx >= 0.0 && cx < (double)a.dim[0] && cy >= 0.0 && cy < (double)a.dim[1] && cz >= 0.0 && cz < (double)a.dim[2];
        if (!inside) { out++; continue; }
        const int cell = (int)cx + a.dim[0] * ((int)cy + a.dim[1] * (int)cz);
        const double v = a.field[cell];
        if (bc < 0 || mapdist_before(v, j, bv, bj)) { bv = v; bj = j; bc = cell; }
    }
    for (int off = 32; off > 0; off >>= 1) {
        const double ov = __shfl_xor(bv, off);
        const int oj = __shfl_xor(bj, off), oc = __shfl_xor(bc, off);
        out += __shfl_xor(out, off);
        if (oc >= 0 && (bc < 0 || mapdist_before(ov, oj, bv, bj))) { bv = ov; bj = oj; bc = oc; }
    }
    if (lane == 0) {
        double *o = a.rows + (size_t)piece * 4;
        o[0] = bc < 0 ? __builtin_huge_val() : bv;
        o[1] = bc < 0 ? -1.0 : step * bj;
        o[2] = (double)bc;
        o[3] = (double)out;
    }
}

} // namespace frx
