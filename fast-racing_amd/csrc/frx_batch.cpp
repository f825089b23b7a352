// The batch entries of the C ABI that take no handle: segment dilation, whole corridors, vertex enumeration, the voxel map's distance field and marking, and the
// tests' sight line.  They have one shape.  A DEVICE form takes device pointers and a stream, checks its arguments and only launches (nothing is allocated, copied
// or waited for: it can be captured in a graph).  A BLOCKING form takes host buffers and a device ordinal: upload, the device form on the null stream, download,
// and - where the device writes fixed-size slots - a host compaction into the CSR the next stage takes.  A blocking form holds its device memory in DevBufs declared
// after its DeviceGuard (frx_hip_scope.hpp), so every exit path frees it and then puts the caller's device back; what it decides on the host is in
// frx_batch_host.hpp, where tests/hostcheck reaches it without a device.  Verdicts come in one order: argument rules, "no HIP device", the device ordinal,
// allocation, HIP errors, capacity.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/frx.h"
#include "../../include/frx_debug.h"
#include "frx_batch_host.hpp"
#include "frx_device.hpp"
#include "frx_esdf_plan.hpp"
#include "frx_hip_scope.hpp"
#include "frx_internal.hpp"
#include "frx_route_host.hpp"
#include "frx_route_window_host.hpp"

namespace {

int invalid(const char *who, const char *what) { return frx::set_error(FRX_ERR_INVALID_ARG, std::string(who) + ": " + what); }
using frx::no_device;
int hip_failed(const char *who, hipError_t e) { return frx::set_error(FRX_ERR_HIP, std::string(who) + ": " + hipGetErrorString(e)); }
template <class T> hipError_t to_device(T *dst, const T *src, size_t n) { return hipMemcpy(dst, src, sizeof(T) * n, hipMemcpyHostToDevice); }
template <class T> hipError_t to_host(T *dst, const T *src, size_t n) { return hipMemcpy(dst, src, sizeof(T) * n, hipMemcpyDeviceToHost); }

// the rules both corridor entries share
int chain_launch_args(const char *who, int n_paths, int n_obs, const double *bbox, double max_seg, const frx_voxel_map *map, int cap_polys, int cap_planes) {
    if (n_paths < 1 || n_obs < 0 || !bbox || cap_polys < 1) return invalid(who, "null or out-of-range argument");
    if (cap_planes < 8) return invalid(who, "cap_planes < 8 (six box planes, floor and ceiling)");
    if (cap_planes > frx::CHAIN_MAX_PLANES) return frx::set_error(FRX_ERR_INVALID_ARG, std::string(who) + ": cap_planes > " + std::to_string((int)frx::CHAIN_MAX_PLANES) + " (a cell's records stay in LDS)");
    if (!(max_seg > 0)) return invalid(who, "max_seg must be above 0");
    if (map) if (int rc = frx::voxel_map_args(map, who, true)) return rc;
    if ((double)n_paths * cap_polys > 2.0e9) return invalid(who, "n_paths x cap_polys exceeds 2e9");
    return FRX_OK;
}

} // namespace

extern "C" {

// Device form of frx_line_segment_dilate for a batch of segments against one obstacle cloud (frx_corridor_kernels.hpp): host
// buffers in and out, one workgroup per segment.  n_planes[s] = number of half-space records of segment s (tangent planes in the
// reference's order, then the six planes of the local box).
int frx_dilate_batch(int device, int n_seg, const double *p1, const double *p2, const double *bbox, int n_obs, const double *obs, double offset,
                     int cap_planes, int *n_planes, double *h_rec, double *ell_C, double *ell_d) {
    const char *who = "frx_dilate_batch";
    if (n_seg < 1 || !p1 || !p2 || !bbox || n_obs < 0 || (n_obs && !obs) || cap_planes < 6 || !n_planes || !h_rec) return invalid(who, "null or out-of-range argument");
    if (frx_device_count() < 1) return no_device();
    DeviceGuard restore_device;
    if (hipSetDevice(device) != hipSuccess) return invalid(who, "device ordinal out of range");
    const size_t S = (size_t)n_seg, n_h = 6 * (size_t)cap_planes * S;
    DevBuf<double> d_p1, d_p2, d_obs, d_h, d_C, d_d;
    DevBuf<int> d_np;
    int rc;
    if ((rc = dev_alloc(d_p1, 3 * S, who)) || (rc = dev_alloc(d_p2, 3 * S, who)) || (rc = dev_alloc(d_obs, 3 * (size_t)std::max(n_obs, 1), who)) ||
        (rc = dev_alloc(d_h, n_h, who)) || (rc = dev_alloc(d_C, 9 * S, who)) || (rc = dev_alloc(d_d, 3 * S, who)) || (rc = dev_alloc(d_np, S, who)))
        return rc;
    hipError_t e = to_device(d_p1.p, p1, 3 * S);
    if (e == hipSuccess) e = to_device(d_p2.p, p2, 3 * S);
    if (e == hipSuccess && n_obs) e = to_device(d_obs.p, obs, 3 * (size_t)n_obs);
    frx::DilateLaunch L;
    L.p1 = d_p1.p; L.p2 = d_p2.p; L.obs = d_obs.p; L.bbox[0] = bbox[0]; L.bbox[1] = bbox[1]; L.bbox[2] = bbox[2]; L.offset = offset;
    L.S = n_seg; L.n_obs = n_obs; L.cap_planes = cap_planes; L.pcap = 4096;              // 4096 candidate points per cell: 96 KB of LDS + flags
    L.n_planes = d_np.p; L.h_rec = d_h.p; L.ell_C = d_C.p; L.ell_d = d_d.p;
    if (e == hipSuccess) e = (hipError_t)frx::launch_dilate(L, nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = to_host(n_planes, d_np.p, S);
    if (e == hipSuccess) e = to_host(h_rec, d_h.p, n_h);
    if (e == hipSuccess && ell_C) e = to_host(ell_C, d_C.p, 9 * S);
    if (e == hipSuccess && ell_d) e = to_host(ell_d, d_d.p, 3 * S);
    if (e != hipSuccess) return hip_failed(who, e);
    for (int s = 0; s < n_seg; s++)
        if (n_planes[s] < 0) return frx::set_error(FRX_ERR_CAPACITY, n_planes[s] == -1 ? "frx_dilate_batch: more than 4096 obstacle points inside one cell's local box"
                                                                                         : "frx_dilate_batch: more half-spaces than cap_planes");
    return FRX_OK;
}

// ---- whole corridors for a batch of paths (frx_chain_kernel.hpp): the device form is one launch, the blocking form is that launch between an upload and a
// host compaction of the slotted records into the CSR frx_problem_create_from_h takes ----
int frx_corridor_generate_batch_device(int n_paths, const int *path_off_dev, const double *path_dev, int n_obs, const double *obs_dev, const double *bbox,
                                       double map_height, double max_seg, const frx_voxel_map *map, int cap_polys, int cap_planes, double *h_slot_dev,
                                       int *cell_planes_dev, int *n_polys_dev, int *status_dev, void *hip_stream) {
    const char *who = "frx_corridor_generate_batch_device";
    if (int rc = chain_launch_args(who, n_paths, n_obs, bbox, max_seg, map, cap_polys, cap_planes)) return rc;
    if (!path_off_dev || !path_dev || (n_obs && !obs_dev) || !h_slot_dev || !cell_planes_dev || !n_polys_dev || !status_dev) return invalid(who, "null argument");
    frx::ChainLaunch L;
    L.path_off = path_off_dev; L.path = path_dev; L.obs = obs_dev;
    for (int i = 0; i < 3; i++) { L.map_origin[i] = map ? map->origin[i] : 0.0; L.map_dim[i] = map ? map->dim[i] : 0; L.bbox[i] = bbox[i]; }
    L.map_res = map ? map->res : 1.0; L.map_cells = map ? map->cells : nullptr;
    L.map_height = map_height; L.max_seg = max_seg;
    L.n_paths = n_paths; L.n_obs = n_obs; L.cap_polys = cap_polys; L.cap_planes = cap_planes; L.pcap = frx::CHAIN_PCAP;
    L.h_slot = h_slot_dev; L.cell_planes = cell_planes_dev; L.n_polys = n_polys_dev; L.status = status_dev;
    const hipError_t e = (hipError_t)frx::launch_chain(L, hip_stream);
    return e == hipSuccess ? FRX_OK : hip_failed(who, e);
}

int frx_corridor_generate_batch(int device, int n_paths, const int *path_off, const double *path, int n_obs, const double *obs, const double *bbox, double map_height,
                                double max_seg, const frx_voxel_map *map, int cap_polys, int cap_planes, int *n_polys, int *status, int cap_rec, int *n_rec,
                                int *h_off, double *h_rec) {
    const char *who = "frx_corridor_generate_batch";
    int rc = chain_launch_args(who, n_paths, n_obs, bbox, max_seg, map, cap_polys, cap_planes);
    if (rc != FRX_OK) return rc;
    if (!path_off || !path || (n_obs && !obs) || !n_polys || !status || !n_rec || !h_off || !h_rec || cap_rec < 0) return invalid(who, "null or out-of-range argument");
    if (path_off[0] < 0) return invalid(who, "path_off[0] < 0");
    for (int b = 0; b < n_paths; b++) {
        if (path_off[b + 1] < path_off[b]) return frx::set_error(FRX_ERR_INVALID_ARG, std::string(who) + ": path_off is not monotone at path " + std::to_string(b));
        if (path_off[b + 1] - path_off[b] < 2) return frx::set_error(FRX_ERR_INVALID_ARG, std::string(who) + ": path " + std::to_string(b) + " has fewer than 2 points");
    }
    if (frx_device_count() < 1) return no_device();
    DeviceGuard restore_device;
    if (hipSetDevice(device) != hipSuccess) return invalid(who, "device ordinal out of range");
    const size_t n_pts = (size_t)path_off[n_paths], n_cells = map ? (size_t)map->dim[0] * map->dim[1] * map->dim[2] : 0;
    const size_t P = (size_t)n_paths, slots = P * cap_polys, cell_doubles = 6 * (size_t)cap_planes;
    DevBuf<int> d_off, d_cp, d_np, d_st;
    DevBuf<double> d_path, d_obs, d_slot;
    DevBuf<signed char> d_cells;
    if ((rc = dev_alloc(d_off, P + 1, who)) || (rc = dev_alloc(d_cp, slots, who)) || (rc = dev_alloc(d_np, P, who)) || (rc = dev_alloc(d_st, P, who)) ||
        (rc = dev_alloc(d_path, 3 * n_pts, who)) || (rc = dev_alloc(d_obs, 3 * (size_t)std::max(n_obs, 1), who)) || (rc = dev_alloc(d_slot, cell_doubles * slots, who)) ||
        (map && (rc = dev_alloc(d_cells, n_cells, who))))
        return rc;
    hipError_t e = to_device(d_off.p, path_off, P + 1);
    if (e == hipSuccess) e = to_device(d_path.p, path, 3 * n_pts);
    if (e == hipSuccess && n_obs) e = to_device(d_obs.p, obs, 3 * (size_t)n_obs);
    if (e == hipSuccess && map) e = to_device(d_cells.p, map->cells, n_cells);
    if (e != hipSuccess) return hip_failed(who, e);
    frx_voxel_map dmap;
    if (map) { dmap = *map; dmap.cells = d_cells.p; }
    rc = frx_corridor_generate_batch_device(n_paths, d_off.p, d_path.p, n_obs, d_obs.p, bbox, map_height, max_seg, map ? &dmap : nullptr, cap_polys, cap_planes, d_slot.p,
                                            d_cp.p, d_np.p, d_st.p, nullptr);
    if (rc != FRX_OK) return rc;
    std::vector<int> cp(slots);
    e = hipStreamSynchronize(nullptr);
    if (e == hipSuccess) e = to_host(n_polys, d_np.p, P);
    if (e == hipSuccess) e = to_host(status, d_st.p, P);
    if (e == hipSuccess) e = to_host(cp.data(), d_cp.p, slots);
    if (e != hipSuccess) return hip_failed(who, e);
    // compaction: the cells of the paths that finished, in path order; of a cell's slot only the widest cell's share of every row of the path is fetched
    long long need = 0;
    for (int b = 0; b < n_paths; b++) need += frx::slots_need(n_polys[b], &cp[(size_t)b * cap_polys]);
    if (!frx::need_fits(need, cap_rec, n_rec))
        return frx::set_error(FRX_ERR_CAPACITY, std::string(who) + ": " + std::to_string(need) + " records, cap_rec is " + std::to_string(cap_rec));
    std::vector<double> stage;
    int poly = 0, used = 0;
    h_off[0] = 0;
    for (int b = 0; b < n_paths; b++) {
        const int *k = &cp[(size_t)b * cap_polys];
        const int nc = n_polys[b];
        if (nc < 1) continue;
        const size_t widest = (size_t)*std::max_element(k, k + nc), row = sizeof(double) * 6 * widest;
        stage.resize(6 * widest * nc);
        e = hipMemcpy2D(stage.data(), row, d_slot.p + (size_t)b * cap_polys * cell_doubles, sizeof(double) * cell_doubles, row, (size_t)nc, hipMemcpyDeviceToHost);
        if (e != hipSuccess) return hip_failed(who, e);
        used = frx::pack_slots(6, nc, k, widest, stage.data(), used, h_rec, h_off + poly);
        poly += nc;
    }
    return FRX_OK;
}

// ---- H -> V vertex enumeration for a batch of polytopes (frx_enumerate_kernel.hpp): the device form is one launch, the blocking form is that launch between
// an upload of the CSR frx_problem_create_from_h takes and a host compaction of the vertex slots into the CSR frx_problem_create takes ----
int frx_enumerate_vertices_batch_device(int n_tasks, const int *tasks_dev, const double *h_rec_dev, int cap_v, double *v_slot_dev, int *nv_dev, int *status_dev,
                                        void *hip_stream) {
    const char *who = "frx_enumerate_vertices_batch_device";
    if (n_tasks < 1 || !tasks_dev || !h_rec_dev || !v_slot_dev || !nv_dev || !status_dev) return invalid(who, "null argument or n_tasks < 1");
    if (cap_v < frx::ENUM_MIN_CAP_V || cap_v > frx::ENUM_MAX_CAP_V) return invalid(who, "cap_v outside [4, 512] (the accepted vertices stay in LDS)");
    if (frx_device_count() < 1) return no_device();
    frx::EnumLaunch L;
    L.tasks = tasks_dev; L.h_rec = h_rec_dev; L.n_tasks = n_tasks; L.cap_v = cap_v; L.v_slot = v_slot_dev; L.nv = nv_dev; L.status = status_dev;
    const hipError_t e = (hipError_t)frx::launch_enumerate(L, hip_stream);
    return e == hipSuccess ? FRX_OK : hip_failed(who, e);
}

int frx_corridor_slots_to_tasks_device(int n_paths, int cap_polys, int cap_planes, const int *cell_planes_dev, const int *n_polys_dev, int *tasks_dev, void *hip_stream) {
    const char *who = "frx_corridor_slots_to_tasks_device";
    if (n_paths < 1 || cap_polys < 1 || cap_planes < 1 || !cell_planes_dev || !n_polys_dev || !tasks_dev) return invalid(who, "null or out-of-range argument");
    if ((double)n_paths * cap_polys * cap_planes > 2.0e9) return invalid(who, "n_paths x cap_polys x cap_planes exceeds 2e9 (record indices are int)");
    if (frx_device_count() < 1) return no_device();
    const hipError_t e = (hipError_t)frx::launch_slots_to_tasks(n_paths, cap_polys, cap_planes, cell_planes_dev, n_polys_dev, tasks_dev, hip_stream);
    return e == hipSuccess ? FRX_OK : hip_failed(who, e);
}

int frx_enumerate_vertices_batch(int device, int B, const int *coarse_n, const int *h_off, const double *h_rec, int cap_v, int *status, int *v_off, int cap_vert,
                                 int *n_vert, double *v_rec) {
    const char *who = "frx_enumerate_vertices_batch";
    if (B < 1 || !coarse_n || !h_off || !h_rec || !status || !v_off || !n_vert || !v_rec || cap_vert < 0) return invalid(who, "null or out-of-range argument");
    if (cap_v < frx::ENUM_MIN_CAP_V || cap_v > frx::ENUM_MAX_CAP_V) return invalid(who, "cap_v outside [4, 512] (the accepted vertices stay in LDS)");
    long long n_poly = 0;
    int rc = frx::enum_csr_args(who, B, coarse_n, h_off, &n_poly);
    if (rc != FRX_OK) return rc;
    if (frx_device_count() < 1) return no_device();
    DeviceGuard restore_device;
    if (hipSetDevice(device) != hipSuccess) return invalid(who, "device ordinal out of range");
    const std::vector<int> tasks = frx::enum_tasks(B, coarse_n, h_off);
    const int NT = (int)(tasks.size() / 4);
    const size_t n_rec = (size_t)h_off[n_poly], slot_doubles = 3 * (size_t)cap_v;
    DevBuf<int> d_tasks, d_nv, d_st;
    DevBuf<double> d_rec, d_slot;
    if ((rc = dev_alloc(d_tasks, tasks.size(), who)) || (rc = dev_alloc(d_nv, NT, who)) || (rc = dev_alloc(d_st, NT, who)) ||
        (rc = dev_alloc(d_rec, 6 * std::max<size_t>(n_rec, 1), who)) || (rc = dev_alloc(d_slot, slot_doubles * NT, who)))
        return rc;
    hipError_t e = to_device(d_tasks.p, tasks.data(), tasks.size());
    if (e == hipSuccess && n_rec) e = to_device(d_rec.p, h_rec, 6 * n_rec);
    if (e != hipSuccess) return hip_failed(who, e);
    rc = frx_enumerate_vertices_batch_device(NT, d_tasks.p, d_rec.p, cap_v, d_slot.p, d_nv.p, d_st.p, nullptr);
    if (rc != FRX_OK) return rc;
    std::vector<int> nv(NT);
    e = hipStreamSynchronize(nullptr);
    if (e == hipSuccess) e = to_host(nv.data(), d_nv.p, NT);
    if (e == hipSuccess) e = to_host(status, d_st.p, NT);
    if (e != hipSuccess) return hip_failed(who, e);
    // compaction: of every slot only the widest polytope's share is fetched
    long long need = 0;
    int widest = 0;
    v_off[0] = 0;
    for (int t = 0; t < NT; t++) { need += nv[t]; widest = std::max(widest, nv[t]); v_off[t + 1] = frx::clip_count(need); }
    if (!frx::need_fits(need, cap_vert, n_vert))
        return frx::set_error(FRX_ERR_CAPACITY, std::string(who) + ": " + std::to_string(need) + " vertices, cap_vert is " + std::to_string(cap_vert));
    if (widest > 0) {
        const size_t row = sizeof(double) * 3 * (size_t)widest;
        std::vector<double> stage((size_t)3 * widest * NT);
        e = hipMemcpy2D(stage.data(), row, d_slot.p, sizeof(double) * slot_doubles, row, (size_t)NT, hipMemcpyDeviceToHost);
        if (e != hipSuccess) return hip_failed(who, e);
        frx::pack_slots(3, NT, nv.data(), (size_t)widest, stage.data(), 0, v_rec, v_off);
    }
    return FRX_OK;
}

// ---- the voxel map's distance field (frx_esdf_kernel.hpp): the device form is five launches, the blocking form is those between an upload and a download ----
int frx_map_esdf_device(const frx_voxel_map *map, double *pos_dev, double *neg_dev, double *all_dev, void *work_dev, void *hip_stream) {
    const char *who = "frx_map_esdf_device";
    if (int rc = frx::esdf_map_args(map, who)) return rc;
    if (!pos_dev && !neg_dev && !all_dev) return invalid(who, "pos, neg and all are all NULL");
    if (!work_dev) return invalid(who, "work_dev is NULL: frx_map_esdf_workspace says how much scratch the launches need");
    if (frx_device_count() < 1) return no_device();
    frx::EsdfLaunch L;
    L.cells = map->cells; L.res = map->res; L.work = work_dev; L.pos = pos_dev; L.neg = neg_dev; L.all = all_dev;
    for (int i = 0; i < 3; i++) L.dim[i] = map->dim[i];
    const hipError_t e = (hipError_t)frx::launch_esdf(L, hip_stream);
    return e == hipSuccess ? FRX_OK : hip_failed(who, e);
}

int frx_map_esdf_on_device(int device, const frx_voxel_map *map, double *pos, double *neg, double *all) {
    const char *who = "frx_map_esdf_on_device";
    if (int rc = frx::esdf_map_args(map, who)) return rc;
    if (!pos && !neg && !all) return invalid(who, "pos, neg and all are all NULL");
    if (frx_device_count() < 1) return no_device();
    DeviceGuard restore_device;
    if (hipSetDevice(device) != hipSuccess) return invalid(who, "device ordinal out of range");
    const frx::EsdfPlan plan = frx::esdf_plan(map->dim);
    const size_t n = (size_t)plan.cells;
    DevBuf<signed char> d_cells;
    DevBuf<unsigned char> d_work;
    DevBuf<double> d_out[3];
    double *host[3] = {pos, neg, all};
    int rc;
    if ((rc = dev_alloc(d_cells, n, who)) || (rc = dev_alloc(d_work, plan.work_bytes, who))) return rc;
    for (int k = 0; k < 3; k++)
        if (host[k] && (rc = dev_alloc(d_out[k], n, who))) return rc;
    hipError_t e = to_device(d_cells.p, map->cells, n);
    if (e != hipSuccess) return hip_failed(who, e);
    frx_voxel_map dmap = *map;
    dmap.cells = d_cells.p;
    rc = frx_map_esdf_device(&dmap, d_out[0].p, d_out[1].p, d_out[2].p, d_work.p, nullptr);
    if (rc != FRX_OK) return rc;
    e = hipStreamSynchronize(nullptr);
    for (int k = 0; k < 3 && e == hipSuccess; k++)
        if (host[k]) e = to_host(host[k], d_out[k].p, n);
    return e == hipSuccess ? FRX_OK : hip_failed(who, e);
}

int frx_map_mark_cloud_device(const frx_voxel_map *map, signed char *cells_dev, int n_pts, const double *pts_dev, int *n_inside_dev, void *hip_stream) {
    const char *who = "frx_map_mark_cloud_device";
    if (!map || !cells_dev || !n_inside_dev || n_pts < 0 || (n_pts > 0 && !pts_dev)) return invalid(who, "null argument or n_pts < 0");
    if (int rc = frx::voxel_map_args(map, who, false)) return rc;
    if (frx_device_count() < 1) return no_device();
    const hipError_t e = (hipError_t)frx::launch_mark_cloud(map->origin, map->dim, map->res, cells_dev, n_pts, pts_dev, n_inside_dev, hip_stream);
    return e == hipSuccess ? FRX_OK : hip_failed(who, e);
}

// ---- a batch of routes through the voxel map (frx_route_kernel.hpp): the device form is four launches, the blocking form is those between an upload and a
// download; the splice into one CSR happens on the device in both ----
int frx_route_plan_batch_device(const frx_voxel_map *map, int n_routes, int n_legs, const int *pt_off_dev, const double *pts_dev, int cap_level, int cap_raw,
                                int cap_pts, int cap_total, void *work_dev, int *path_off_dev, double *path_dev, int *route_status_dev, int *leg_status_dev,
                                int *leg_levels_dev, int *leg_max_level_dev, void *hip_stream) {
    const char *who = "frx_route_plan_batch_device";
    if (!pt_off_dev || !pts_dev || !work_dev || !path_off_dev || !path_dev || !route_status_dev || !leg_status_dev || !leg_levels_dev || !leg_max_level_dev)
        return invalid(who, "null argument");
    if (int rc = frx::route_batch_args(map, who, n_routes, cap_level, cap_raw, cap_pts, cap_total)) return rc;
    if (n_legs < n_routes) return invalid(who, "n_legs < n_routes (every route has at least two waypoints)");
    if ((size_t)work_dev % 8 != 0) return invalid(who, "work_dev is not 8-byte aligned (the workspace begins with doubles and its labels are cleared as 64-bit words)");
    if (frx::route_work(map->dim, n_legs, cap_level, cap_raw, cap_pts).verdict != frx::ROUTE_WORK_FITS)
        return frx::set_error(FRX_ERR_CAPACITY, std::string(who) + ": the workspace exceeds 4e18 bytes");
    if (frx_device_count() < 1) return no_device();
    frx::RouteLaunch L;
    for (int i = 0; i < 3; i++) { L.origin[i] = map->origin[i]; L.dim[i] = map->dim[i]; }
    L.res = map->res; L.cells = map->cells; L.pt_off = pt_off_dev; L.pts = pts_dev;
    L.n_routes = n_routes; L.n_legs = n_legs; L.cap_level = cap_level; L.cap_raw = cap_raw; L.cap_pts = cap_pts; L.cap_total = cap_total;
    L.work = work_dev; L.path_off = path_off_dev; L.path = path_dev; L.route_status = route_status_dev; L.leg_status = leg_status_dev;
    L.leg_levels = leg_levels_dev; L.leg_max_level = leg_max_level_dev;
    const hipError_t e = (hipError_t)frx::launch_route(L, hip_stream);
    return e == hipSuccess ? FRX_OK : hip_failed(who, e);
}

// The blocking form of both searches: leg_window NULL is the whole-map search; otherwise the search inside per-leg windows, whose rows come back in leg_window.
static int route_blocking(const char *who, int device, const frx_voxel_map *map, int n_routes, const int *pt_off, const double *pts, int pad, long long cap_window,
                          int cap_level, int cap_raw, int cap_pts, int cap_total, int *path_off, double *path, int *route_status, int *leg_status, int *leg_levels,
                          int *leg_max_level, int *leg_window, int *n_pts) {
    if (!pt_off || !pts || !path_off || !path || !route_status || !leg_status || !leg_levels || !leg_max_level || !n_pts) return invalid(who, "null argument");
    if (int rc = frx::route_batch_args(map, who, n_routes, cap_level, cap_raw, cap_pts, cap_total)) return rc;
    if (leg_window)
        if (int rc = frx::route_window_args(who, pad, cap_window)) return rc;
    long long legs = 0;
    if (int rc = frx::route_offset_args(who, n_routes, pt_off, &legs)) return rc;
    const frx::RouteWork w = leg_window ? frx::route_window_work(legs, cap_level, cap_raw, cap_pts, cap_window) : frx::route_work(map->dim, legs, cap_level, cap_raw, cap_pts);
    if (w.verdict != frx::ROUTE_WORK_FITS) return frx::set_error(FRX_ERR_CAPACITY, std::string(who) + ": the workspace exceeds 4e18 bytes");
    if (frx_device_count() < 1) return no_device();
    DeviceGuard restore_device;
    if (hipSetDevice(device) != hipSuccess) return invalid(who, "device ordinal out of range");
    const size_t R = (size_t)n_routes, NL = (size_t)legs, n_wp = (size_t)pt_off[n_routes], n_cells = (size_t)map->dim[0] * map->dim[1] * map->dim[2];
    DevBuf<signed char> d_cells;
    DevBuf<unsigned char> d_work;
    DevBuf<int> d_off, d_poff, d_rst, d_lst, d_lev, d_max, d_win;
    DevBuf<double> d_pts, d_path;
    int rc;
    if ((rc = dev_alloc(d_cells, n_cells, who)) || (rc = dev_alloc(d_work, w.bytes, who)) || (rc = dev_alloc(d_off, R + 1, who)) || (rc = dev_alloc(d_poff, R + 1, who)) ||
        (rc = dev_alloc(d_rst, R, who)) || (rc = dev_alloc(d_lst, NL, who)) || (rc = dev_alloc(d_lev, NL, who)) || (rc = dev_alloc(d_max, NL, who)) ||
        (leg_window && (rc = dev_alloc(d_win, 8 * NL, who))) || (rc = dev_alloc(d_pts, 3 * n_wp, who)) || (rc = dev_alloc(d_path, 3 * (size_t)cap_total, who)))
        return rc;
    hipError_t e = to_device(d_cells.p, map->cells, n_cells);
    if (e == hipSuccess) e = to_device(d_off.p, pt_off, R + 1);
    if (e == hipSuccess) e = to_device(d_pts.p, pts, 3 * n_wp);
    if (e != hipSuccess) return hip_failed(who, e);
    frx_voxel_map dmap = *map;
    dmap.cells = d_cells.p;
    rc = leg_window ? frx_route_plan_window_batch_device(&dmap, n_routes, (int)legs, d_off.p, d_pts.p, pad, cap_window, cap_level, cap_raw, cap_pts, cap_total, d_work.p,
                                                         d_poff.p, d_path.p, d_rst.p, d_lst.p, d_lev.p, d_max.p, d_win.p, nullptr)
                    : frx_route_plan_batch_device(&dmap, n_routes, (int)legs, d_off.p, d_pts.p, cap_level, cap_raw, cap_pts, cap_total, d_work.p, d_poff.p, d_path.p,
                                                  d_rst.p, d_lst.p, d_lev.p, d_max.p, nullptr);
    if (rc != FRX_OK) return rc;
    std::vector<int> npts(NL);
    e = hipStreamSynchronize(nullptr);
    if (e == hipSuccess) e = to_host(path_off, d_poff.p, R + 1);
    if (e == hipSuccess) e = to_host(route_status, d_rst.p, R);
    if (e == hipSuccess) e = to_host(leg_status, d_lst.p, NL);
    if (e == hipSuccess) e = to_host(leg_levels, d_lev.p, NL);
    if (e == hipSuccess) e = to_host(leg_max_level, d_max.p, NL);
    if (e == hipSuccess && leg_window) e = to_host(leg_window, d_win.p, 8 * NL);
    if (e == hipSuccess) e = to_host(npts.data(), (const int *)(d_work.p + w.npts_off), NL);
    if (e == hipSuccess && path_off[n_routes] > 0) e = to_host(path, d_path.p, 3 * (size_t)path_off[n_routes]);
    if (e != hipSuccess) return hip_failed(who, e);
    // the room all routes would take: a route with a failed leg takes its placeholder whatever the room
    long long need = 0;
    for (int r = 0, leg = 0; r < n_routes; r++) {
        const int nl = pt_off[r + 1] - pt_off[r] - 1;
        bool whole = true;
        for (int l = 0; l < nl; l++) whole = whole && leg_status[leg + l] == 0;
        need += whole ? frx::route_points(nl, &npts[leg]) : 2;
        leg += nl;
    }
    if (!frx::need_fits(need, cap_total, n_pts))
        return frx::set_error(FRX_ERR_CAPACITY, std::string(who) + ": " + std::to_string(need) + " points, cap_total is " + std::to_string(cap_total));
    return FRX_OK;
}

int frx_route_plan_batch(int device, const frx_voxel_map *map, int n_routes, const int *pt_off, const double *pts, int cap_level, int cap_raw, int cap_pts,
                         int cap_total, int *path_off, double *path, int *route_status, int *leg_status, int *leg_levels, int *leg_max_level, int *n_pts) {
    return route_blocking("frx_route_plan_batch", device, map, n_routes, pt_off, pts, -1, 0, cap_level, cap_raw, cap_pts, cap_total, path_off, path, route_status, leg_status,
                          leg_levels, leg_max_level, nullptr, n_pts);
}

// ---- the same batch inside certified per-leg windows (frx_route_window_kernel.hpp): three launches, the labels of a leg sized by cap_window, not by the map ----
int frx_route_plan_window_batch_device(const frx_voxel_map *map, int n_routes, int n_legs, const int *pt_off_dev, const double *pts_dev, int pad,
                                       long long cap_window, int cap_level, int cap_raw, int cap_pts, int cap_total, void *work_dev, int *path_off_dev,
                                       double *path_dev, int *route_status_dev, int *leg_status_dev, int *leg_levels_dev, int *leg_max_level_dev,
                                       int *leg_window_dev, void *hip_stream) {
    const char *who = "frx_route_plan_window_batch_device";
    if (!pt_off_dev || !pts_dev || !work_dev || !path_off_dev || !path_dev || !route_status_dev || !leg_status_dev || !leg_levels_dev || !leg_max_level_dev ||
        !leg_window_dev)
        return invalid(who, "null argument");
    if (int rc = frx::route_batch_args(map, who, n_routes, cap_level, cap_raw, cap_pts, cap_total)) return rc;
    if (int rc = frx::route_window_args(who, pad, cap_window)) return rc;
    if (n_legs < n_routes) return invalid(who, "n_legs < n_routes (every route has at least two waypoints)");
    if ((size_t)work_dev % 8 != 0) return invalid(who, "work_dev is not 8-byte aligned (the workspace begins with doubles)");
    if (frx::route_window_work(n_legs, cap_level, cap_raw, cap_pts, cap_window).verdict != frx::ROUTE_WORK_FITS)
        return frx::set_error(FRX_ERR_CAPACITY, std::string(who) + ": the workspace exceeds 4e18 bytes");
    if (frx_device_count() < 1) return no_device();
    frx::RouteWindowLaunch W;
    frx::RouteLaunch &L = W.r;
    for (int i = 0; i < 3; i++) { L.origin[i] = map->origin[i]; L.dim[i] = map->dim[i]; }
    L.res = map->res; L.cells = map->cells; L.pt_off = pt_off_dev; L.pts = pts_dev;
    L.n_routes = n_routes; L.n_legs = n_legs; L.cap_level = cap_level; L.cap_raw = cap_raw; L.cap_pts = cap_pts; L.cap_total = cap_total;
    L.work = work_dev; L.path_off = path_off_dev; L.path = path_dev; L.route_status = route_status_dev; L.leg_status = leg_status_dev;
    L.leg_levels = leg_levels_dev; L.leg_max_level = leg_max_level_dev;
    W.pad = pad; W.cap_window = cap_window; W.leg_window = leg_window_dev;
    const hipError_t e = (hipError_t)frx::launch_route_window(W, hip_stream);
    return e == hipSuccess ? FRX_OK : hip_failed(who, e);
}

int frx_route_plan_window_batch(int device, const frx_voxel_map *map, int n_routes, const int *pt_off, const double *pts, int pad, long long cap_window,
                                int cap_level, int cap_raw, int cap_pts, int cap_total, int *path_off, double *path, int *route_status, int *leg_status,
                                int *leg_levels, int *leg_max_level, int *leg_window, int *n_pts) {
    const char *who = "frx_route_plan_window_batch";
    if (!leg_window) return invalid(who, "null argument");
    return route_blocking(who, device, map, n_routes, pt_off, pts, pad, cap_window, cap_level, cap_raw, cap_pts, cap_total, path_off, path, route_status, leg_status,
                          leg_levels, leg_max_level, leg_window, n_pts);
}

// Tests: the device's sight line (map_blocked, frx_chain_kernel.hpp) on n_pairs pairs of points, host buffers in and out; out[i] = 0 / 1 as frx_map_is_blocked.
int frx_debug_map_blocked_device(int device, const frx_voxel_map *map, int n_pairs, const double *a, const double *b, int *out) {
    const char *who = "frx_debug_map_blocked_device";
    if (!map || n_pairs < 1 || !a || !b || !out) return invalid(who, "null or out-of-range argument");
    if (int rc = frx::voxel_map_args(map, who, true)) return rc;
    if (frx_device_count() < 1) return no_device();
    DeviceGuard restore_device;
    if (hipSetDevice(device) != hipSuccess) return invalid(who, "device ordinal out of range");
    const size_t n = (size_t)n_pairs, n_cells = (size_t)map->dim[0] * map->dim[1] * map->dim[2];
    DevBuf<double> d_a, d_b;
    DevBuf<int> d_out;
    DevBuf<signed char> d_cells;
    int rc;
    if ((rc = dev_alloc(d_a, 3 * n, who)) || (rc = dev_alloc(d_b, 3 * n, who)) || (rc = dev_alloc(d_out, n, who)) || (rc = dev_alloc(d_cells, n_cells, who))) return rc;
    hipError_t e = to_device(d_a.p, a, 3 * n);
    if (e == hipSuccess) e = to_device(d_b.p, b, 3 * n);
    if (e == hipSuccess) e = to_device(d_cells.p, map->cells, n_cells);
    frx::ChainLaunch L{};
    for (int i = 0; i < 3; i++) { L.map_origin[i] = map->origin[i]; L.map_dim[i] = map->dim[i]; }
    L.map_res = map->res; L.map_cells = d_cells.p;
    if (e == hipSuccess) e = (hipError_t)frx::launch_map_blocked_pairs(L, n_pairs, d_a.p, d_b.p, d_out.p, nullptr);
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    if (e == hipSuccess) e = to_host(out, d_out.p, n);
    return e == hipSuccess ? FRX_OK : hip_failed(who, e);
}

} // extern "C"
