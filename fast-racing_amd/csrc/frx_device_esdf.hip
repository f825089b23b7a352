// hipcc translation unit of the voxel map's device side: its distance field and the marking of a cloud (frx_esdf_kernel.hpp), the screen of a batch of
// trajectories against a field (frx_mapdist_kernel.hpp), and their launchers.  Built without contraction (Makefile): cell indices are rounded quotients and the
// combined field rounds pos before the sum.
#include <hip/hip_runtime.h>

#include "frx_esdf_kernel.hpp"
#include "frx_mapdist_kernel.hpp"

namespace frx {

int launch_esdf(const EsdfLaunch &e, void *stream) {
    const EsdfPlan plan = esdf_plan(e.dim);
    if (plan.verdict != ESDF_FITS || !e.cells || !e.work || !(e.pos || e.neg || e.all)) return (int)hipErrorInvalidValue;
    EsdfArgs a;
    a.cells = e.cells; a.nx = e.dim[0]; a.ny = e.dim[1]; a.nz = e.dim[2]; a.ncol = (int)plan.columns; a.n = (int)plan.cells; a.res = e.res;
    int *w = (int *)e.work;
    a.gz_occ = w; a.gz_free = w + plan.cells; a.gy_occ = w + 2 * plan.cells; a.gy_free = w + 3 * plan.cells; a.flag = w + plan.flag_off;
    a.yd_occ = w + plan.ydist_off; a.yd_free = a.yd_occ + plan.columns;
    a.want_occ = (e.pos || e.all) ? 1 : 0; a.want_free = (e.neg || e.all) ? 1 : 0;
    a.pos = e.pos; a.neg = e.neg; a.all = e.all;
    const hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_esdf_flags, dim3(plan.grid_flags), dim3(ESDF_THREADS), 0, s, a.flag, a.nx + 1);
    hipLaunchKernelGGL(k_esdf_z, dim3(plan.grid_z), dim3(ESDF_THREADS), 0, s, a);
    hipLaunchKernelGGL(k_esdf_ycol, dim3(plan.grid_ycol), dim3(ESDF_THREADS), 0, s, a);
    hipLaunchKernelGGL(k_esdf_y, dim3(plan.grid_y), dim3(ESDF_THREADS), 0, s, a);
    hipLaunchKernelGGL(k_esdf_x, dim3(plan.grid_x), dim3(ESDF_THREADS), plan.lds_x, s, a);
    return (int)hipGetLastError();
}

int launch_mark_cloud(const double *origin, const int *dim, double res, signed char *cells, int n_pts, const double *pts, int *n_inside, void *stream) {
    if (!cells || !n_inside || n_pts < 0 || (n_pts && !pts)) return (int)hipErrorInvalidValue;
    MarkArgs a;
    for (int i = 0; i < 3; i++) { a.origin[i] = origin[i]; a.dim[i] = dim[i]; }
    a.res = res; a.cells = cells; a.pts = pts; a.n_pts = n_pts; a.n_inside = n_inside;
    hipLaunchKernelGGL(k_mark_zero, dim3(1), dim3(1), 0, (hipStream_t)stream, n_inside);
    if (n_pts > 0) hipLaunchKernelGGL(k_mark_cloud, dim3((n_pts + ESDF_THREADS - 1) / ESDF_THREADS), dim3(ESDF_THREADS), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

int launch_map_distance(int P, const double *T, const double *C, int intervals, const double *origin, const int *dim, double res, const double *field,
                        double *rows, void *stream) {
    if (P < 1 || intervals < 1 || !T || !C || !field || !rows) return (int)hipErrorInvalidValue;
    MapDistArgs a;
    for (int i = 0; i < 3; i++) { a.origin[i] = origin[i]; a.dim[i] = dim[i]; }
    a.res = res; a.field = field; a.T = T; a.C = C; a.P = P; a.M = intervals; a.rows = rows;
    const int per_wg = MAPDIST_THREADS / 64;
    hipLaunchKernelGGL(k_traj_map_distance, dim3((P + per_wg - 1) / per_wg), dim3(MAPDIST_THREADS), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

} // namespace frx
