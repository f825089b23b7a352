// hipcc translation unit of the route batch (frx_route_kernel.hpp), its form inside per-leg windows (frx_route_window_kernel.hpp) and their launchers.  Built without contraction (Makefile): cell indices are rounded quotients and
// samplePath's points fall on cell faces.
#include <hip/hip_runtime.h>

#include "frx_device.hpp"
#include "frx_route_kernel.hpp"
#include "frx_route_window_kernel.hpp"

namespace frx {

int launch_route(const RouteLaunch &r, void *stream) {
    const RouteWork w = route_work(r.dim, r.n_legs, r.cap_level, r.cap_raw, r.cap_pts);
    if (w.verdict != ROUTE_WORK_FITS || r.n_routes < 1 || r.n_legs < r.n_routes || (long long)r.cap_total < 2LL * r.n_routes || !r.cells || !r.pt_off || !r.pts ||
        !r.work || !r.path_off || !r.path || !r.route_status || !r.leg_status || !r.leg_levels || !r.leg_max_level)
        return (int)hipErrorInvalidValue;
    RouteArgs a;
    for (int i = 0; i < 3; i++) { a.origin[i] = r.origin[i]; a.dim[i] = r.dim[i]; }
    a.res = r.res; a.cells = r.cells; a.pt_off = r.pt_off; a.pts = r.pts;
    a.n_routes = r.n_routes; a.n_legs = r.n_legs; a.cap_level = r.cap_level; a.cap_raw = r.cap_raw; a.cap_pts = r.cap_pts; a.cap_total = r.cap_total;
    a.label_words = (unsigned)w.label_words;
    char *base = (char *)r.work;
    a.slot = (double *)(base + w.slot_off); a.npts = (int *)(base + w.npts_off); a.lists = (int *)(base + w.list_off); a.labels = (unsigned *)(base + w.label_off);
    a.path_off = r.path_off; a.path = r.path; a.route_status = r.route_status; a.leg_status = r.leg_status; a.leg_levels = r.leg_levels;
    a.leg_max_level = r.leg_max_level;
    const hipStream_t s = (hipStream_t)stream;
    const size_t n64 = (w.bytes - w.label_off) / 8;                              // the label region ends the workspace and is padded to 8 bytes
    const size_t blocks = (n64 + ROUTE_THREADS - 1) / ROUTE_THREADS;
    hipLaunchKernelGGL(k_route_clear, dim3((unsigned)(blocks < 8192 ? (blocks ? blocks : 1) : 8192)), dim3(ROUTE_THREADS), 0, s, (unsigned long long *)a.labels, n64);
    hipLaunchKernelGGL(k_route_search, dim3(r.n_legs), dim3(ROUTE_THREADS), 0, s, a);
    hipLaunchKernelGGL(k_route_splice_plan, dim3(1), dim3(ROUTE_THREADS), 0, s, a);
    hipLaunchKernelGGL(k_route_splice, dim3(r.n_routes), dim3(ROUTE_THREADS), 0, s, a);
    return (int)hipGetLastError();
}

int launch_route_window(const RouteWindowLaunch &wl, void *stream) {
    const RouteLaunch &r = wl.r;
    const RouteWork w = route_window_work(r.n_legs, r.cap_level, r.cap_raw, r.cap_pts, wl.cap_window);
    const long long layer = r.dim[0] > 0 && r.dim[1] > 0 ? (long long)r.dim[0] * r.dim[1] : 0;
    if (w.verdict != ROUTE_WORK_FITS || r.dim[2] <= 0 || layer < 1 || layer > 0x7fffffffLL || layer * r.dim[2] > 0x7fffffffLL || wl.pad < 0 ||
        wl.pad > ROUTE_PAD_MAX || r.n_routes < 1 || r.n_legs < r.n_routes || (long long)r.cap_total < 2LL * r.n_routes || !r.cells || !r.pt_off || !r.pts || !r.work ||
        !r.path_off || !r.path || !r.route_status || !r.leg_status || !r.leg_levels || !r.leg_max_level || !wl.leg_window)
        return (int)hipErrorInvalidValue;
    RouteWindowArgs wa;
    RouteArgs &a = wa.r;
    for (int i = 0; i < 3; i++) { a.origin[i] = r.origin[i]; a.dim[i] = r.dim[i]; }
    a.res = r.res; a.cells = r.cells; a.pt_off = r.pt_off; a.pts = r.pts;
    a.n_routes = r.n_routes; a.n_legs = r.n_legs; a.cap_level = r.cap_level; a.cap_raw = r.cap_raw; a.cap_pts = r.cap_pts; a.cap_total = r.cap_total;
    a.label_words = (unsigned)w.label_words;
    char *base = (char *)r.work;
    a.slot = (double *)(base + w.slot_off); a.npts = (int *)(base + w.npts_off); a.lists = (int *)(base + w.list_off); a.labels = (unsigned *)(base + w.label_off);
    a.path_off = r.path_off; a.path = r.path; a.route_status = r.route_status; a.leg_status = r.leg_status; a.leg_levels = r.leg_levels;
    a.leg_max_level = r.leg_max_level;
    wa.pad = wl.pad; wa.cap_window = wl.cap_window; wa.leg_window = wl.leg_window;
    const hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_route_search_window, dim3(r.n_legs), dim3(ROUTE_THREADS), 0, s, wa);
    hipLaunchKernelGGL(k_route_splice_plan, dim3(1), dim3(ROUTE_THREADS), 0, s, a);
    hipLaunchKernelGGL(k_route_splice, dim3(r.n_routes), dim3(ROUTE_THREADS), 0, s, a);
    return (int)hipGetLastError();
}

} // namespace frx
