/*
 * frx.h — C ABI of the MI355X-native back-end for Fast-Racing's SE(3) MINCO optimiser.
 *
 * This is the drop-in boundary.  Every entry point names the reference
 * interface it replaces; paths are relative to /root/reference/src/plan_manage/:
 *   CPU.hpp = include/se3gcopter/se3gcopter_cpu.hpp     GPU.hpp = include/se3gcopter/se3gcopter_gpu.hpp
 *   cc.cuh  = include/cuda_computer.cuh                 cc.cu   = src/cuda_computer.cu
 *   lbfgs.hpp = include/se3gcopter/lbfgs.hpp
 *
 * Conventions
 *   - plain pointers and sizes only; no exceptions cross the ABI; every call returns an int
 *     status (0 = FRX_OK, <0 = error, see frx_status) and frx_last_error() gives the text.
 *   - all floating point is IEEE binary64, exactly like the reference.
 *   - a problem handle holds a BATCH of B independent candidate trajectories (the reference
 *     has B = 1); candidates may have different piece counts and different
 *     numbers of free variables.  Per-candidate quantities are packed back to back and
 *     addressed through the offset arrays returned by frx_problem_layout().
 *   - 3x3 boundary states are column-major (p | v | a), as Eigen stores the reference's
 *     iniState/finState (se3_node_cpu.cpp:98-99, CPU.hpp:440-442).
 *   - coefficient blocks are (6N x 3) ROW-major per candidate: row 6i+k = coefficient of t^k
 *     of piece i (CPU.hpp:244,260); i.e. piece-major, 18 contiguous doubles per piece.
 *   - "_device" variants take device pointers and a hipStream_t (passed as void*) and are
 *     asynchronous; the plain variants take host pointers and block.
 *   - the library never falls back to a CPU implementation: without a usable HIP device
 *     frx_problem_create() fails with FRX_ERR_NO_DEVICE.
 *   - diagnostics (traces, in-kernel profiles, self-tests of single kernels) are NOT part of this boundary: include/frx_debug.h.
 */
#ifndef FRX_H
#define FRX_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FRX_VERSION 100

typedef enum frx_status {
    FRX_OK = 0,
    FRX_ERR_INVALID_ARG = -1,
    FRX_ERR_NO_DEVICE = -2,        /* no usable HIP device (there is no CPU fallback) */
    FRX_ERR_HIP = -3,              /* HIP runtime error later on */
    FRX_ERR_EMPTY_POLYTOPE = -4,   /* a corridor cell or overlap has no vertices: SE3GCOPTER::setup returns false (CPU.hpp:1118-1121) */
    FRX_ERR_CAPACITY = -5,         /* piece count too large for the LDS-resident band (reference silently caps N <= 100, cc.cuh:24) */
    FRX_ERR_ALLOC = -6,            /* host or device allocation failed (at create or later) */
    FRX_ERR_TIMEOUT = -7           /* a bounded wait on the device expired (FRX_ROUND_TIMEOUT_MS, default 5000); the handle stays usable */
} frx_status;

/* Scalar arguments of SE3GCOPTER::setup (CPU.hpp:1076-1092), named after the ROS parameters
 * that feed them (se3_planner.h:61-98, misc/zhangjiajie_params.yaml). */
typedef struct frx_config {
    double rho;             /* Rho        > 0: soft total time, weight of sum(T) (CPU.hpp:1097-1102) */
    double total_t;         /* TotalT     used only when rho <= 0 */
    double grid_res;        /* gridRes    INFINITY at the only call site (MinCoPlan_CPU.cpp:117) */
    int qd_intervals;       /* QdIntervals = kappa, trapezoid intervals per piece */
    int c2_diffeo;          /* UseC2Diffeo */
    double horiz_half_len;  /* HorizHalfLen  ellipsoid semi-axes (x, y) */
    double vert_half_len;   /* VertHalfLen   ellipsoid semi-axis z */
    double safe_margin;     /* SafeMargin */
    double vel_max;         /* VelMax */
    double thr_acc_min;     /* ThrustAccMin */
    double thr_acc_max;     /* ThrustAccMax */
    double body_rate_max;   /* BodyRateMax */
    double grav_acc;        /* GravAcc */
    double penalty_pvtb[4]; /* PenaltyPVTB  weights: corridor, velocity, thrust (both bounds), body rate */
} frx_config;

/* L-BFGS parameters = lbfgs::lbfgs_parameter_t (lbfgs.hpp:18-140), same defaults. */
typedef struct frx_lbfgs_params {
    int mem_size;
    double g_epsilon;
    int past;
    double delta;
    int max_iterations;
    int max_linesearch;
    double min_step;
    double max_step;
    double f_dec_coeff;
    double s_curv_coeff;
    double xtol;
} frx_lbfgs_params;

typedef struct frx_problem frx_problem;

int frx_version(void);
/* Text of the last error raised on this thread (never NULL). */
const char *frx_last_error(void);
/* Number of usable HIP devices (0 when there is none; never fails). */
int frx_device_count(void);

/* Fills p with lbfgs_load_default_parameters (lbfgs.hpp:1040-1043). */
void frx_lbfgs_default_params(frx_lbfgs_params *p);
/* Fills p with the values SE3GCOPTER::optimize uses (CPU.hpp:1243-1247): mem_size 128, past 3,
 * g_epsilon 1e-16, min_step 1e-32, delta = rel_cost_tol, everything else default. */
void frx_lbfgs_gcopter_params(frx_lbfgs_params *p, double rel_cost_tol);

/*
 * Replaces SE3GCOPTER::setup (CPU.hpp:1076-1186) + cuda_computer::setup (cc.cu:413-466) for a
 * batch of B candidates on HIP device `device`.  Everything that is constant during the
 * optimisation (polytopes, index maps, boundary states, parameters) is uploaded ONCE here;
 * the reference re-packs ~257 KB through mapped memory on every evaluation (cc.cu:492-527).
 *
 *   coarse_n[B]            polytopes (= coarse pieces) per candidate
 *   ini_state, fin_state   B x 9 doubles, column-major 3x3 (p | v | a) per candidate
 *   h_off, h_rec           CSR over ALL candidates' H-polytopes in order: polytope m owns the
 *                          half-space records h_off[m] .. h_off[m+1]-1, 6 doubles each
 *                          (outer normal, point) = one column of the reference's 6 x K matrix
 *                          (MinCoPlan_CPU.cpp:93-105).  Normals are re-normalised (CPU.hpp:1116).
 *   v_off, v_rec           CSR over ALL candidates' V-polytopes; candidate b owns 2*coarse_n[b]-1
 *                          of them in the order [cell 0, overlap 0|1, cell 1, ...] (CPU.hpp:1031-1074);
 *                          3 doubles per vertex.  These are the OUTPUT of geoutils::enumerateVs,
 *                          which stays on the caller's side for now; the
 *                          [v0, v_r - v0] re-basing of CPU.hpp:1049 is done inside.
 */
int frx_problem_create(const frx_config *cfg, int device, int B, const int *coarse_n,
                       const double *ini_state, const double *fin_state,
                       const int *h_off, const double *h_rec,
                       const int *v_off, const double *v_rec,
                       frx_problem **out);
/*
 * Same, but the V-polytopes are enumerated here from the H-polytopes (cells and consecutive overlaps), replacing
 * SE3GCOPTER::extractVs -> geoutils::enumerateVs (CPU.hpp:1031-1074, geoutils.hpp:43-149): the caller passes exactly what
 * MavGlobalPlanner::plan passes to setup (MinCoPlan_CPU.cpp:93-123).  Vertices are ordered lexicographically (the
 * reference's order depends on a process-global RNG; any fixed order parameterises the same polytope).
 * Fails with FRX_ERR_EMPTY_POLYTOPE when a cell or an overlap has no interior (setup() == false, CPU.hpp:1118-1121).
 */
int frx_problem_create_from_h(const frx_config *cfg, int device, int B, const int *coarse_n,
                              const double *ini_state, const double *fin_state,
                              const int *h_off, const double *h_rec, frx_problem **out);
/* Vertices (3 doubles each, lexicographic order) of one H-polytope given as K records (outer normal, point). */
int frx_enumerate_vertices(int K, const double *h_rec, double *v_out, int cap, int *nv);

/* The same enumeration on the DEVICE for a batch of polytopes (csrc/frx_enumerate_kernel.hpp): one 256-thread workgroup per task walks the plane triples in
 * the host's order in windows of 256, keeps the first triple of every 1e-7 grid key, sorts by key and judges the polytope - vertices, counts and verdicts are
 * those of frx_enumerate_vertices / frx_problem_create_from_h bit for bit (every operation is the host's, in its order, none fused).
 * A task = {begin0, count0, begin1, count1}, four int in records of 6 doubles: the polytope's planes are records begin0 .. begin0+count0-1 followed by
 * begin1 .. begin1+count1-1 (a cell: count1 = 0; an overlap: the two cells' ranges, which need not be contiguous); count0 = 0: no task.
 * status per task (FRX_HV_*): 0 = ok; 1 = unbounded and 2 = flat, the host's two refusals (FRX_ERR_EMPTY_POLYTOPE there) - nv and the vertices are written as
 * the host computes them; 3 = fewer than 4 or more than 256 planes; 4 = more distinct vertices than cap_v; 5 = a record is not finite; 6 = no task.  For 3 - 6
 * nv = 0 and the task's vertices are left untouched.  A task does not disturb another; the call returns FRX_OK whatever the statuses are.
 *   frx_enumerate_vertices_batch          blocking, host pointers; takes what frx_problem_create_from_h takes, builds the 2 coarse_n[b] - 1 tasks of every
 *                                         candidate in the order [cell 0, overlap 0|1, cell 1, ...], and compacts the result into the CSR frx_problem_create
 *                                         takes: status[n_tasks], v_off[n_tasks + 1], v_rec[3 cap_vert].  *n_vert = vertices needed; FRX_ERR_CAPACITY only when
 *                                         that exceeds cap_vert (status and v_off are valid then).
 *   frx_enumerate_vertices_batch_device   ONE launch on hip_stream of the current device: no copy, no synchronisation, no allocation (capturable).  Device
 *                                         pointers; outputs v_slot[n_tasks][cap_v][3], nv[n_tasks], status[n_tasks].  The caller vouches for the tasks' ranges.
 *   frx_corridor_slots_to_tasks_device    ONE launch of index arithmetic: tasks[n_paths][2 cap_polys - 1] from the outputs of
 *                                         frx_corridor_generate_batch_device, record indices into h_slot viewed as one record array (cell c of path p starts at
 *                                         (p cap_polys + c) cap_planes); positions beyond a path's 2 n_polys - 1 get count0 = 0.  So corridors -> tasks ->
 *                                         vertices runs on one stream without the host.
 * FRX_ERR_INVALID_ARG (reported before a device is looked for): NULL arguments, B / n_tasks / n_paths < 1, a coarse_n[b] < 1, non-monotone h_off, cap_v outside
 * [4, 512] (the accepted vertices stay in LDS), cap_polys or cap_planes < 1.  FRX_ERR_NO_DEVICE without a device.  Not built: an O(K^3) edge-clipping
 * enumeration - it would meet other duplicates in another order and lose the bit-for-bit referee. */
enum { FRX_HV_OK = 0, FRX_HV_UNBOUNDED = 1, FRX_HV_FLAT = 2, FRX_HV_PLANES = 3, FRX_HV_VERTICES = 4, FRX_HV_NONFINITE = 5, FRX_HV_SKIPPED = 6 };
#define FRX_HV_MAX_PLANES 256
int frx_enumerate_vertices_batch(int device, int B, const int *coarse_n, const int *h_off, const double *h_rec, int cap_v, int *status, int *v_off,
                                 int cap_vert, int *n_vert, double *v_rec);
int frx_enumerate_vertices_batch_device(int n_tasks, const int *tasks_dev, const double *h_rec_dev, int cap_v, double *v_slot_dev, int *nv_dev,
                                        int *status_dev, void *hip_stream);
int frx_corridor_slots_to_tasks_device(int n_paths, int cap_polys, int cap_planes, const int *cell_planes_dev, const int *n_polys_dev, int *tasks_dev,
                                       void *hip_stream);

/* Safe-flight-corridor generation, the step upstream of frx_problem_create_from_h.
 * frx_line_segment_dilate = LineSegment3D::dilate(offset) (decomp_util/line_segment.h:31-35 with find_ellipsoid :136-214,
 * DecompBase::find_polyhedron decomp_base.h:63-83, add_local_bbox line_segment.h:47-85, obstacle filter decomp_base.h:35-40):
 * the cell of segment p1-p2 in the point cloud obs[3 n_obs] as (normal, point) records in the reference's order (planes tangent at
 * points that lie ON the final ellipsoid tie at distance 1 and rounding orders them), optionally
 * the inflated ellipsoid (C row-major 3x3, centre d).  Pass h_rec = NULL to query *n_planes.
 * frx_corridor_generate = the corridor loop of MavGlobalPlanner::plan (MinCoPlan_CPU.cpp:37-105): cells chained greedily along
 * path[3 n_path] (segments shorter than max_seg = 4 m and not `blocked`, restart at 4/5 of the in-cell span), floor and ceiling
 * planes z in [0, map_height] appended; output in the CSR layout frx_problem_create takes.  `blocked` replaces
 * MapUtil::isBlocked (map_util.h:417) and may be NULL (nothing blocks). */
typedef int (*frx_blocked_fn)(const double *a, const double *b, void *user);
int frx_line_segment_dilate(const double *p1, const double *p2, const double *bbox, int n_obs, const double *obs, double offset,
                            int cap, int *n_planes, double *h_rec, double *ell_C, double *ell_d);
int frx_corridor_generate(int n_path, const double *path, int n_obs, const double *obs, const double *bbox, double map_height,
                          double max_seg, frx_blocked_fn blocked, void *user, int cap_polys, int cap_planes, int *n_polys,
                          int *h_off, double *h_rec);

/* The same cell on the DEVICE for a batch of segments against one obstacle cloud (csrc/frx_corridor_kernels.hpp): one workgroup per segment,
 * the candidate points compacted in cloud order into LDS, every step of find_ellipsoid / find_polyhedron (decomp_util line_segment.h:136-214,
 * decomp_base.h:63-83) = an arg-min and a filter over them on 256 lanes.  p1, p2: n_seg x 3; h_rec: n_seg x cap_planes x 6 (outer normal, point),
 * n_planes[s] records of it valid (tangent planes in the reference's order, then the six planes of the local box); ell_C (n_seg x 9),
 * ell_d (n_seg x 3) may be NULL.  FRX_ERR_CAPACITY when a cell's local box holds more than 4096 points or needs more than cap_planes planes:
 * n_planes[s] is then -1 (points) or -2 (planes) for every such segment, whose rows of h_rec, ell_C and ell_d are undefined; every other segment's
 * n_planes and rows are valid and are what the call gives without the refused segments. */
int frx_dilate_batch(int device, int n_seg, const double *p1, const double *p2, const double *bbox, int n_obs, const double *obs, double offset,
                     int cap_planes, int *n_planes, double *h_rec, double *ell_C, double *ell_d);

/* Whole corridors on the DEVICE for a batch of independent paths against one obstacle cloud and one voxel map (csrc/frx_chain_kernel.hpp): what
 * frx_corridor_generate computes for one path with blocked = frx_map_is_blocked, one 256-thread workgroup per path walking that path's greedy chain
 * (segment end by length and sight line, the cell as frx_dilate_batch forms it with offset 0, exit index, floor and ceiling, restart at 4/5 of the in-cell
 * span).  path_off[n_paths + 1] = first point of every path in path[3 path_off[n_paths]]; obs as frx_dilate_batch takes it; map = NULL: nothing blocks.
 * A path's result depends on that path, the cloud and the map alone and is bit-identical run to run, in either form and in any batch.
 * status[b]: 0 = ok; 1 = a cell's local box holds more than 4096 cloud points; 2 = a cell needs more than cap_planes records (floor and ceiling included);
 * 3 = more than cap_polys cells.  A path with a non-zero status has n_polys[b] = 0 and does not disturb the others; the call still returns FRX_OK.
 *   frx_corridor_generate_batch          blocking, host pointers (map->cells on the host); uploads paths, cloud and cells, then compacts the slots into ONE
 *                                        CSR over all paths in path order: h_off[sum(n_polys) + 1] (room for n_paths x cap_polys + 1 entries), h_rec[6 cap_rec],
 *                                        floor and ceiling last in each cell - the layout frx_problem_create_from_h takes with coarse_n = n_polys.
 *                                        *n_rec = records needed; FRX_ERR_CAPACITY only when that exceeds cap_rec (n_polys and status are valid then).
 *   frx_corridor_generate_batch_device   ONE launch on hip_stream of the current device: no copy, no synchronisation, no allocation (capturable).  All array
 *                                        arguments but bbox are device pointers, map is a host struct whose cells point to device memory.  Slotted outputs:
 *                                        h_slot[n_paths][cap_polys][cap_planes][6], cell_planes[n_paths][cap_polys] (records of each cell), n_polys, status;
 *                                        slots beyond a path's cells are left untouched.  The caller vouches for path_off (every path >= 2 points, monotone).
 * FRX_ERR_INVALID_ARG (reported before a device is looked for): NULL arguments, n_paths < 1, a path with fewer than 2 points, non-monotone path_off,
 * cap_polys < 1, cap_planes < 8 or > 512 (a cell's records stay in LDS beside its 4096 candidate points), max_seg not above 0, a map with res <= 0 or a
 * dim <= 0.  FRX_ERR_NO_DEVICE without a device.  Not built (csrc/frx_chain_kernel.hpp): a spatial index over the cloud, and a split of one path's
 * cloud scans over several workgroups - one path runs on one compute unit. */
struct frx_voxel_map;                                                 /* defined below, with the path-search front end */
int frx_corridor_generate_batch(int device, int n_paths, const int *path_off, const double *path, int n_obs, const double *obs, const double *bbox,
                                double map_height, double max_seg, const struct frx_voxel_map *map, int cap_polys, int cap_planes, int *n_polys, int *status,
                                int cap_rec, int *n_rec, int *h_off, double *h_rec);
int frx_corridor_generate_batch_device(int n_paths, const int *path_off_dev, const double *path_dev, int n_obs, const double *obs_dev, const double *bbox,
                                       double map_height, double max_seg, const struct frx_voxel_map *map, int cap_polys, int cap_planes, double *h_slot_dev,
                                       int *cell_planes_dev, int *n_polys_dev, int *status_dev, void *hip_stream);

/* Result wire format.  frx_traj_to_msg fills the array fields of quadrotor_msgs/PolynomialTrajectory the way
 * MavGlobalPlanner::traj2msg does (se3_planner.cpp:31-58): per piece 6 duration-normalised coefficients per axis, highest
 * power first (Piece::normalizePosCoeffMat, trajectory.hpp:131-141), time[] = durations, order[] = 5 (num_order = 5,
 * mag_coeff = 1, action = ACTION_ADD are constants of that function).  frx_msg_sample evaluates such a message at time t
 * after its start exactly like traj_server (traj_server.cpp:406-456): position, velocity, acceleration, jerk. */
int frx_traj_to_msg(int n_pieces, const double *T, const double *C, double *coef_x, double *coef_y, double *coef_z,
                    double *time, unsigned *order);
int frx_msg_sample(int n_segment, const double *coef_x, const double *coef_y, const double *coef_z, const double *time,
                   const unsigned *order, double t, double *pos, double *vel, double *acc, double *jerk);

/* Path-search front end on the voxel grid -- the step of MavGlobalPlanner::plan that produces the polyline
 * frx_corridor_generate takes (MinCoPlan_CPU.cpp:13-35).  The searches that return the reference's OWN path (frx_grid_search,
 * frx_jps_plan, frx_route_plan: its heap order, JPS, any eps) are host code (csrc/frx_search.cpp); a batch of routes that needs
 * a shortest path of the reference's length, not that very path, is searched on the device (frx_route_plan_batch below).
 * frx_voxel_map = what JPS::MapUtil<3> holds (map_util.h:48-75, setMap :365): cell (i,j,k) covers
 * origin + [i,i+1) x [j,j+1) x [k,k+1) * res, stored x fastest; 0 = free, 100 = occupied, -1 = unknown (:322-327). */
typedef struct frx_voxel_map {
    double origin[3];
    int dim[3];
    double res;
    const signed char *cells;
} frx_voxel_map;
/* MapUtil::GlobalMapBuild / setObs (map_util.h:86-136): mark the cells holding the cloud's points occupied (points outside
 * the map are dropped).  Returns the number of points inside (>= 0) or a negative frx_status. */
int frx_map_mark_cloud(const double *origin, const int *dim, double res, int n_pts, const double *pts, signed char *cells);
/* MapUtil::isBlocked (map_util.h:395-425) with the signature of frx_blocked_fn: pass it to frx_corridor_generate with
 * user = the frx_voxel_map.  1 when a cell at or above 100 lies on the 0.8-cell ray walk strictly between a and b. */
int frx_map_is_blocked(const double *a, const double *b, void *map);
/* The Euclidean distance field of the map: MapUtil::updateESDF3d / fillESDF (map_util.h:149-278), the buffers getDistance reads (:309-318).  A cell with
 * cells > 0 is occupied (isOccupied, :326), one with cells == 0 is free (:322), one with cells == -1 is neither.  Over the grid, x fastest:
 *   pos[c] = res sqrt(d2_occ[c])    d2_occ = the exact squared distance in cells, an integer, from cell c to the nearest occupied cell (0 on one)
 *   neg[c] = res sqrt(d2_free[c])   likewise to the nearest free cell
 *   all[c] = pos[c], and where neg[c] > 0.0, all[c] = pos[c] + (-neg[c] + res) with the parenthesis first (:241-243)
 * Every double is fully determined - one correctly rounded square root, one product, for all two sums in that order, none of it fused - so the forms agree bit
 * for bit, run to run and inside a graph.  One deliberate difference from the reference: its arithmetic on DBL_MAX gives res sqrt(DBL_MAX) where a map holds no
 * site of a kind at all; here such a field is +inf, and the combine rule's IEEE outcome stands: all = -inf where only neg is infinite, NaN (the quiet NaN with a clear sign and no payload) where both are.
 * Any of pos, neg, all may be NULL and is then not computed (all three NULL: FRX_ERR_INVALID_ARG).
 *   frx_map_esdf             host code on one thread (csrc/frx_esdf_host.hpp): the reference's three lower-envelope passes on integer values; the referee
 *                            of the device form.
 *   frx_map_esdf_workspace   bytes of scratch the device form needs for a grid of dim[3]: a function of dim alone, answered without a device.
 *   frx_map_esdf_device      pure launches on hip_stream of the current device (csrc/frx_esdf_kernel.hpp): no copy, no synchronisation, no allocation
 *                            (capturable).  map is a host struct whose cells point to device memory; pos_dev, neg_dev, all_dev, work_dev are device pointers.
 *   frx_map_esdf_on_device   blocking, host pointers: upload, the device form, download.
 * FRX_ERR_INVALID_ARG, reported before a device is looked for: a NULL map, cells, dim or work_dev, res not above 0, a dim <= 0.  FRX_ERR_CAPACITY, likewise: a
 * dim[1] or dim[2] above 16384 (3 dim^2 stays inside 31 bits), a dim[0] above 8192 (the x pass keeps a line in LDS), more than 2^31 - 1 cells.
 * FRX_ERR_NO_DEVICE without a device (the device forms).  Not built: the distance-map planner that reads the field in the reference. */
int frx_map_esdf(const frx_voxel_map *map, double *pos, double *neg, double *all);
int frx_map_esdf_workspace(const int *dim, size_t *bytes);
int frx_map_esdf_device(const frx_voxel_map *map, double *pos_dev, double *neg_dev, double *all_dev, void *work_dev, void *hip_stream);
int frx_map_esdf_on_device(int device, const frx_voxel_map *map, double *pos, double *neg, double *all);
/* frx_map_mark_cloud on the DEVICE (setObs, map_util.h:108-136): pure launches on hip_stream, capturable.  map gives origin, dim and res (its cells are not
 * read); cells_dev (the grid), pts_dev (n_pts x 3) and n_inside_dev (one int: the points inside) are device pointers.  The cell rule is map_blocked's,
 * round((p - origin) / res - 0.5), none of it fused; the stores are bytes of 100, so racing ones are harmless, and the count is a sum of integers.
 * FRX_ERR_INVALID_ARG (before a device is looked for): NULL arguments (pts_dev with n_pts == 0 excepted), n_pts < 0, res not above 0, a dim <= 0, more than
 * 2^31 - 1 cells. */
int frx_map_mark_cloud_device(const frx_voxel_map *map, signed char *cells_dev, int n_pts, const double *pts_dev, int *n_inside_dev, void *hip_stream);
/* JPS::GraphSearch::plan (graph_search.h:129-161, graph_search.cpp:79-236) on a dense occupancy array cmap (0 = free, > 0 =
 * occupied, x fastest): A* (use_jps = 0; six face neighbours in 3-D, eight in 2-D -- the only mode plan_manage calls,
 * MinCoPlan_CPU.cpp:15) or jump-point search (26 / 8 neighbours) with heuristic eps * Euclidean distance.  dim[2] = 0 selects
 * the 2-D search.  The path comes back goal first, as GraphSearch::getPath() holds it, cell for cell the one the reference
 * returns (same successor order, comparator and heap steps).  *n_path = 0 when the goal is unreachable or max_expand (> 0)
 * expansions were spent; *cost = g of the goal.  FRX_ERR_CAPACITY when the path holds more than cap cells. */
int frx_grid_search(const signed char *cmap, const int *dim, const int *start, const int *goal, double eps, int use_jps,
                    int max_expand, int cap, int *n_path, int *path_xyz, int *n_expanded, double *cost);
/* JPSPlanner<3>::plan (jps_planner.cpp:333-420): cells of start and goal (must be free: *status = 1 / 2), grid search on the
 * occupied/not-occupied view of the map (unknown cells are traversable, updateMap :309-323), *status = -1 when there is no
 * path; then raw_path (cell centres, start first), path (removeCornerPts forwards and backwards, removeLinePts; :54-117) and
 * sample_path (the centres of the cells the simplified path crosses, samplePath :118-148 = getSamplePath()).  Any output may
 * be NULL; each holds up to cap points (3 doubles). */
int frx_jps_plan(const frx_voxel_map *map, const double *start, const double *goal, double eps, int use_jps, int cap, int *n_raw,
                 double *raw_path, int *n_path, double *path, int *n_sample, double *sample_path, int *status, int *n_expanded);
/* The route of MavGlobalPlanner::plan through the gates (MinCoPlan_CPU.cpp:13-35): legs start -> gate 0 -> ... -> goal,
 * each one frx_jps_plan's sample path, spliced with the shared point kept once.  Legs are independent and run on n_threads
 * host threads (0 = one per core).  leg_status[n_gates + 1] as *status above; when a leg fails *n_out = 0 (the reference
 * splices stale samples there). */
int frx_route_plan(const frx_voxel_map *map, const double *start, const double *goal, int n_gates, const double *gates, double eps,
                   int use_jps, int n_threads, int cap, int *n_out, double *path_out, int *leg_status, int *leg_expanded);
/* A BATCH of routes through the map, searched on the device (csrc/frx_route_kernel.hpp).  The reference's plan mode is A* with eps = 1 over the six
 * face neighbours at unit step cost: the length of its path is the breadth-first distance, an integer, and only WHICH of the equally short paths comes back
 * depends on the order of its heap operations.  These entries return one well-defined path of that length instead, the canonical level search
 * (csrc/frx_route_host.hpp): level 0 is the goal's cell, level L + 1 every traversable (inside, cells <= 0: unknown cells are crossed), unlabelled face neighbour
 * of a level-L cell, built whole until a level labels the start's cell; the path descends from the start, each step to the face neighbour one level down whose
 * squared cell distance to the goal (64-bit integers) is smallest, ties in the order -x, -y, -z, +z, +y, +x.  Then frx_jps_plan's tail, the same operations in the
 * same order: removeCornerPts forwards and backwards, removeLinePts, samplePath.  Host and device forms agree bit for bit.
 * Route r has the waypoints pts[pt_off[r] .. pt_off[r + 1]) - start, gates in order, goal - at least two; its legs are the consecutive pairs, all legs of all routes
 * are independent.  An end of a leg is a cell of the map or outside it, decided on the rounded quotient before it becomes an integer: a coordinate beyond the
 * map, infinite or not a number is outside, and an end outside is not free.  Per leg (in route order): leg_status = 0 ok; 1 start not free; 2 goal not free; -1 no path; 3 a level holds more than cap_level cells; 4 the
 * raw path holds more than cap_raw cells; 5 more than cap_pts sample points.  leg_levels = the start's level (the raw path holds that many cells plus one), -1
 * when the search did not label the start; leg_max_level = the largest level built, the last one included (level 0 counts).  A failed leg does not disturb any
 * other leg and the call still returns FRX_OK.
 * The routes come back as one CSR in route order, path_off[n_routes + 1] and path[cap_total][3], the layout frx_corridor_generate_batch_device takes: the legs'
 * sample paths with the shared point kept once.  route_status = 0 whole; 1 a leg failed; 2 the route does not fit the room left in cap_total once every later
 * route has kept room for two points; 3 fewer than two waypoints (device form only).  A route with a non-zero status gets a two-point placeholder, its first and
 * last waypoint as given, so the CSR stays valid for the corridor kernel; the caller reads the status.  The device form, which cannot refuse what it has not
 * read: a route of ONE waypoint gets status 3 and that waypoint twice, and no other route is disturbed; a route WITHOUT a waypoint (or offsets that step back)
 * leaves fewer leg slots than legs, so the whole batch is refused on the device - every route_status 3 with its placeholder (zeros for the route without a
 * waypoint), every leg_status -1, leg_levels -1, leg_max_level 0 - and every entry of every output is written.  A whole route of one leg whose start and goal
 * share a cell has ONE point.
 *   frx_grid_search_levels        host: the search alone on an occupancy array, as frx_grid_search takes it (3-D only).  The path comes back START first;
 *                                 *n_path = 0, *levels = -1 when there is none (an occupied start or goal included).  levels, max_level_cells may be NULL.
 *   frx_route_plan_levels_batch   host, one thread: the whole batch; the referee of the device form.
 *   frx_route_search_workspace    bytes of scratch the device form needs: per leg cap_pts points, two lists of cap_level cells, cap_raw cells and one label
 *                                 byte per map cell.  A function of its arguments alone, answered without a device.
 *   frx_route_plan_batch_device   pure launches on hip_stream of the current device (four kernels: label clear, search and tail, splice offsets, splice): no
 *                                 copy, no synchronisation, no allocation (capturable).  map is a host struct whose cells point to device memory; every other
 *                                 pointer is a device pointer.  n_legs = pt_off[n_routes] - pt_off[0] - n_routes; the caller vouches for pt_off.
 *                                 work_dev holds frx_route_search_workspace bytes and is 8-byte aligned (FRX_ERR_INVALID_ARG otherwise).
 *   frx_route_plan_batch          blocking, host pointers: upload, the device form, download.
 * The batch forms report in *n_pts the points all routes need and return FRX_ERR_CAPACITY only when that exceeds cap_total (every output is valid then).
 * FRX_ERR_INVALID_ARG (reported before a device is looked for): NULL arguments, n_routes < 1, a route with fewer than two waypoints, non-monotone pt_off, a cap
 * < 1, cap_total < 2 n_routes, res <= 0, a dim <= 0, more than 2^31 - 1 cells.  FRX_ERR_NO_DEVICE without a device (the device forms).  Not built: 2-bit labels,
 * one leg split over several workgroups, JPS and eps != 1 (frx_grid_search, frx_jps_plan and frx_route_plan keep those).  For maps too large for
 * one label byte per cell and leg, frx_route_plan_window_batch below searches inside per-leg windows. */
int frx_grid_search_levels(const signed char *cmap, const int *dim, const int *start, const int *goal, int cap, int *n_path, int *path_xyz, int *levels,
                           int *max_level_cells);
int frx_route_plan_levels_batch(const frx_voxel_map *map, int n_routes, const int *pt_off, const double *pts, int cap_level, int cap_raw, int cap_pts,
                                int cap_total, int *path_off, double *path, int *route_status, int *leg_status, int *leg_levels, int *leg_max_level,
                                int *n_pts);
int frx_route_search_workspace(const int *dim, int n_legs, int cap_level, int cap_raw, int cap_pts, size_t *bytes);
int frx_route_plan_batch_device(const frx_voxel_map *map, int n_routes, int n_legs, const int *pt_off_dev, const double *pts_dev, int cap_level, int cap_raw,
                                int cap_pts, int cap_total, void *work_dev, int *path_off_dev, double *path_dev, int *route_status_dev, int *leg_status_dev,
                                int *leg_levels_dev, int *leg_max_level_dev, void *hip_stream);
int frx_route_plan_batch(int device, const frx_voxel_map *map, int n_routes, const int *pt_off, const double *pts, int cap_level, int cap_raw, int cap_pts,
                         int cap_total, int *path_off, double *path, int *route_status, int *leg_status, int *leg_levels, int *leg_max_level, int *n_pts);
/* The same batch searched INSIDE CERTIFIED PER-LEG WINDOWS of the map (csrc/frx_route_window_kernel.hpp, csrc/frx_route_window_host.hpp), so that a
 * leg's label memory is cap_window bytes whatever the map's size and its flood ends near the leg.  The window of a leg with end cells s, g is the box of s and g
 * widened by pad cells on every side and clipped to the map.  A side on the map's face is closed (nothing lies beyond it); any other side is open and lies
 * exactly pad cells from the box of s, g; a window without an open side is the whole map.  With M = |s - g|_1 a path that leaves through an open side holds at
 * least M + 2 (pad + 1) steps, so a start labelled at a level <= limit = M + 2 pad by the search confined to the window certifies that no shortest path of the
 * whole map leaves it: the leg's path, leg_levels and sample points are then bit for bit those of frx_route_plan_batch.  Otherwise the leg says so and returns no
 * path.  Per leg, beside the statuses above: leg_status = 6 the window holds more than cap_window cells (no label is touched: leg_levels -1, leg_max_level 0);
 * 7 the window is open and the search inside it certifies nothing (a level came out empty, or limit levels were built without labelling the start: no leg
 * builds more than limit levels); -1 is returned only by a window that is the whole map.  The order of the verdicts: 1, 2, 6, then per level 3, found, -1 / 7
 * for an empty level, 7 at the limit; then 4 and 5.  A leg with status 6 or 7 is a failed leg to the splice (route_status 1, the two-point placeholder).
 * leg_max_level is the largest level built inside the window and may be smaller than the whole-map entries' value, also where the path is identical.
 * leg_window [n_legs][8] ints: lo xyz, size xyz, limit (-1 for a whole-map window), 0; every row is written, zeros for a leg whose ends are not free cells
 * (status 1, 2).  The entries above never return 6 or 7.
 *   frx_route_plan_levels_window_batch   host, one thread: the referee of the device form.
 *   frx_route_window_workspace           bytes of scratch the device form needs: per leg 24 cap_pts + 4 + 4 (2 cap_level + cap_raw) + 4 ceil(cap_window / 4),
 *                                        the regions 8-byte aligned.  A function of its arguments alone - the map's size does not enter - answered without a device.
 *   frx_route_plan_window_batch_device   pure launches on hip_stream of the current device (three kernels: search and tail, splice offsets, splice; each
 *                                        workgroup of the search clears the labels of its own window, so work_dev needs no preparation and a replayed graph
 *                                        clears again): no copy, no synchronisation, no allocation (capturable).  Pointer conventions, n_legs, the alignment of
 *                                        work_dev and the rule for a batch with a route without a waypoint as frx_route_plan_batch_device (the leg_window rows
 *                                        of a batch refused that way are written and carry no meaning).
 *   frx_route_plan_window_batch          blocking, host pointers: upload, the device form, download.
 * *n_pts and FRX_ERR_CAPACITY as above.  FRX_ERR_INVALID_ARG (reported before a device is looked for) as above, and for pad < 0, pad > 1 << 20, cap_window < 1,
 * cap_window > 2^31 - 4 (window-local cell indices stay below 2^31).  Not built: labels in LDS for windows small enough to fit, 2-bit labels. */
int frx_route_plan_levels_window_batch(const frx_voxel_map *map, int n_routes, const int *pt_off, const double *pts, int pad, long long cap_window, int cap_level,
                                       int cap_raw, int cap_pts, int cap_total, int *path_off, double *path, int *route_status, int *leg_status, int *leg_levels,
                                       int *leg_max_level, int *leg_window, int *n_pts);
int frx_route_window_workspace(int n_legs, int cap_level, int cap_raw, int cap_pts, long long cap_window, size_t *bytes);
int frx_route_plan_window_batch_device(const frx_voxel_map *map, int n_routes, int n_legs, const int *pt_off_dev, const double *pts_dev, int pad,
                                       long long cap_window, int cap_level, int cap_raw, int cap_pts, int cap_total, void *work_dev, int *path_off_dev,
                                       double *path_dev, int *route_status_dev, int *leg_status_dev, int *leg_levels_dev, int *leg_max_level_dev,
                                       int *leg_window_dev, void *hip_stream);
int frx_route_plan_window_batch(int device, const frx_voxel_map *map, int n_routes, const int *pt_off, const double *pts, int pad, long long cap_window,
                                int cap_level, int cap_raw, int cap_pts, int cap_total, int *path_off, double *path, int *route_status, int *leg_status,
                                int *leg_levels, int *leg_max_level, int *leg_window, int *n_pts);

/* Asynchronous evaluation on host buffers (blocking and asynchronous variants): frx_objective_eval_async returns once
 * the work is enqueued on the handle's stream, frx_wait completes it and fills f and g (valid until then; one evaluation in flight per
 * handle).  The *_device entry points are asynchronous on the caller's stream by construction. */
int frx_objective_eval_async(frx_problem *p, const double *x, double *f, double *g);
int frx_wait(frx_problem *p);

/* Post-checks of a result (MinCoPlan_CPU.cpp:131-132): the largest speed and the largest acceleration magnitude of every piece,
 * Piece::getMaxVelRate / getMaxAccRate (trajectory.hpp:177-273; Trajectory::getMaxVelRate/getMaxAccRate = the max over pieces).
 * T[n_pieces], C[n_pieces][6][3] as frx_optimize returns them; either output may be NULL. */
int frx_traj_max_rates(int n_pieces, const double *T, const double *C, double *max_vel, double *max_acc);

/* Dense feasibility certificate of a batch of results, on the device that holds the handle's corridors.  The reference judges a result by
 * getMaxVelRate / getMaxAccRate alone (MinCoPlan_CPU.cpp:131-132; checkMaxVelRate / checkMaxAccRate, trajectory.hpp:275-315, are never
 * called) and never checks the SE(3) constraints it optimises against; the penalty samples them at kappa + 1 nodes per piece only
 * (CPU.hpp:188-408), so a trajectory can leave its corridor or break a limit between the nodes and still score zero.
 * Every fine piece is sampled at s_j = j (T / M), j = 0..M, M = intervals (1..FRX_CHECK_MAX_INTERVALS; the penalty's abscissa form, so at
 * M = kappa both sample the same points) with the reference's definitions (CPU.hpp:260-299, 322-328, 347-398): h = a + g e3,
 * R = [xB yB zB](h), E = diag(ellipsoid).  Fields of a row (FRX_CHECK_FIELDS doubles):
 *   FRX_CHECK_CORRIDOR    max over j and the piece's half-spaces k of n_k.(p - p_k) + |E R^T n_k|: how far the body reaches past a face,
 *                         WITHOUT safeMargin (<= 0: inside)
 *   FRX_CHECK_SPEED       max |v|        FRX_CHECK_THRUST_MIN  min |h|        FRX_CHECK_THRUST_MAX  max |h|
 *   FRX_CHECK_BODY_RATE   max |omega_xy|, omega_xy = (xB.j, yB.j) / |h| (the quantity the body-rate penalty limits)
 *   FRX_CHECK_ACC         max |a| (the sampled counterpart of getMaxAccRate)
 *   FRX_CHECK_WORST_T     local time s_j of the worst CORRIDOR sample (lowest j on ties)
 *   FRX_CHECK_WORST_K     index k of its half-space within the piece's polytope (lowest k on ties)
 * A candidate's row reduces its pieces in piece order (max; min for THRUST_MIN); there WORST_T is the time from the candidate's start and
 * WORST_K the local index of the piece.  A non-finite sample makes its field NaN (never hidden by a max).  Rows are bit-identical run to
 * run and independent of the rest of the batch.  Flags per candidate, against the handle's own limits with no slack: FRX_CHECK_FLAG_*.
 *   frx_trajectory_check        blocking: T[total fine pieces], C[total fine pieces x 18] on the host as frx_optimize returns them;
 *                               piece_out (P x 8) and flags (B) may be NULL, cand_out (B x 8) may not.
 *   frx_trajectory_check_device a pure launch on the caller's stream (no copy, no synchronisation): piece rows only, device pointers.
 * Serves both kinds of handle (frx_problem_create[_from_h], frx_penalty_problem_create).  FRX_ERR_CAPACITY when a piece's corridor has
 * too many half-spaces for the kernel's LDS (several hundred). */
#define FRX_CHECK_MAX_INTERVALS 16384
#define FRX_CHECK_FIELDS 8
#define FRX_CHECK_CORRIDOR 0
#define FRX_CHECK_SPEED 1
#define FRX_CHECK_THRUST_MIN 2
#define FRX_CHECK_THRUST_MAX 3
#define FRX_CHECK_BODY_RATE 4
#define FRX_CHECK_ACC 5
#define FRX_CHECK_WORST_T 6
#define FRX_CHECK_WORST_K 7
#define FRX_CHECK_FLAG_CORRIDOR 1u      /* CORRIDOR > 0 */
#define FRX_CHECK_FLAG_SPEED 2u         /* SPEED > vel_max */
#define FRX_CHECK_FLAG_THRUST_MIN 4u    /* THRUST_MIN < thr_acc_min */
#define FRX_CHECK_FLAG_THRUST_MAX 8u    /* THRUST_MAX > thr_acc_max */
#define FRX_CHECK_FLAG_BODY_RATE 16u    /* BODY_RATE > body_rate_max */
#define FRX_CHECK_FLAG_NONFINITE 32u    /* a non-finite value in the candidate's row */
int frx_trajectory_check(frx_problem *p, const double *T, const double *C, int intervals, double *piece_out, double *cand_out, unsigned *flags);
int frx_trajectory_check_device(frx_problem *p, const double *T_dev, const double *C_dev, int intervals, double *piece_out_dev, void *hip_stream);

/* Exact extrema of the four dynamic quantities of a batch of results, on the device.  frx_trajectory_check samples, so a limit broken between two of
 * its samples is reported as kept; these entries do not sample.  Under the flatness map of CPU.hpp:260-299 |v|^2, |a|^2 and |h|^2 = |a + g e3|^2
 * are polynomials in t and omega_xy^2 = |h x j|^2 / |h|^4 (j = dh/dt) is a rational function of t, so a piece's extrema are values at the roots of
 * a known polynomial - the derivative of the squared norm; N'Q - 2NQ' (degree 13) for omega_xy^2 = N / Q^2 - and at the piece's two ends.  The
 * roots are found as frx_traj_max_rates finds them (every sign change on the piece, bracketed by the derivative's roots and bisected down to
 * adjacent doubles).  Fields of a row (FRX_EXTREMA_FIELDS doubles):
 *   FRX_EXTREMA_SPEED       max |v|        FRX_EXTREMA_ACC         max |a|
 *   FRX_EXTREMA_THRUST_MIN  min |h|        FRX_EXTREMA_THRUST_MAX  max |h|
 *   FRX_EXTREMA_BODY_RATE   max |omega_xy| (the quantity the body-rate penalty and FRX_CHECK_BODY_RATE limit)
 *   FRX_EXTREMA_T_SPEED .. FRX_EXTREMA_T_BODY_RATE   the local time in [0, T] at which each of the five is attained, in the same order: the
 *                           first one in the order (roots ascending, then 0, then T) on ties
 * SPEED and ACC are frx_traj_max_rates' numbers bit for bit wherever that function does not take its early-out.  It returns 0 for a piece whose
 * |v|^2 (|a|^2) has a numerically zero derivative - the reference's rule, trajectory.hpp:192-195 - so a piece of constant velocity (3, -4, 0)
 * reports speed 0 there; a certificate must not, so here the two ends are always candidates and that piece reports 5 at time 0.  A piece whose T
 * is not finite or <= 0, or that has a coefficient that is not finite, has all ten fields NaN (frx_traj_max_rates drops a NaN in its max and
 * reports 0); a value that is not a number - the body rate where h = 0 - makes its field NaN.
 * A candidate's row reduces its pieces in piece order (max; min for THRUST_MIN; the first piece wins a tie, NaN propagates); its times count
 * from the candidate's start.  Flags per candidate: FRX_CHECK_FLAG_SPEED / THRUST_MIN / THRUST_MAX / BODY_RATE / NONFINITE against the handle's
 * own limits with no slack (ACC is not limited).  The corridor is NOT covered: the body's reach past a face is not polynomial in t; judge it
 * with frx_trajectory_check or, exactly, frx_trajectory_contain; the obstacle cloud itself with frx_trajectory_clearance_exact, which samples nothing
 * either (frx_trajectory_clearance is its dense form).  Rows are bit-identical run to run and independent of the rest of the batch.
 *   frx_trajectory_extrema        blocking: T[total fine pieces], C[total fine pieces x 18] on the host as frx_optimize returns them;
 *                                 piece_out (P x 10) and flags (B) may be NULL, cand_out (B x 10) may not.
 *   frx_trajectory_extrema_device a pure launch on the caller's stream (no copy, no synchronisation, no allocation): piece rows only, device pointers.
 * Serves both kinds of handle.  FRX_ERR_INVALID_ARG for a NULL argument, reported before a device is looked for; FRX_ERR_NO_DEVICE without one. */
#define FRX_EXTREMA_FIELDS 10
#define FRX_EXTREMA_SPEED 0
#define FRX_EXTREMA_ACC 1
#define FRX_EXTREMA_THRUST_MIN 2
#define FRX_EXTREMA_THRUST_MAX 3
#define FRX_EXTREMA_BODY_RATE 4
#define FRX_EXTREMA_T_SPEED 5
#define FRX_EXTREMA_T_ACC 6
#define FRX_EXTREMA_T_THRUST_MIN 7
#define FRX_EXTREMA_T_THRUST_MAX 8
#define FRX_EXTREMA_T_BODY_RATE 9
int frx_trajectory_extrema(frx_problem *p, const double *T, const double *C, double *piece_out, double *cand_out, unsigned *flags);
int frx_trajectory_extrema_device(frx_problem *p, const double *T_dev, const double *C_dev, double *piece_out_dev, void *hip_stream);

/* Exact gate passage certificate of a batch of results, on the device.  The reference reads four corner poses per gate and keeps their mean
 * (se3_node_cpu.cpp:44-61); the centres are way-points of the path search (MinCoPlan_CPU.cpp:13-35) and nothing checks afterwards that the result flies
 * through a gate.  The corridors of frx_trajectory_check are dilated cells round the searched path, not the gate openings.  These entries answer, for
 * every (candidate, gate): does the candidate cross the gate's plane, when, inside the opening with how much room for the body at the attitude it has
 * there, and in gate order.
 * A gate record is 9 doubles {c[3], a[3], b[3]}: the opening is {c + s a + t b : |s| <= 1, |t| <= 1}, a and b the half-edge vectors; the caller vouches
 * that they are orthogonal.  Derived, one correctly rounded operation after the other: wu = |a|, wv = |b|, eu = a / wu, ev = b / wv, m = a x b,
 * n = m / |m| (divisions by the norm, no reciprocal).  Candidate b owns the gates gate_off[b] .. gate_off[b + 1] - 1 in the order they are to be
 * flown; a candidate may own none.
 * Crossings.  On every piece, in normalised time tau = t / T with w_k = c_k T^k, f(tau) = n.(w_0 - c) + sum_{k >= 1} (n.w_k) tau^k is a quintic; its
 * roots on [0, 1] are found as frx_trajectory_extrema finds roots (every sign change, bracketed by the derivative's roots and bisected down to adjacent
 * doubles): the crossing instants are exact, nothing is sampled.  A root that is exactly tau == 0 is dropped unless the piece is the candidate's first:
 * a knot on the plane counts once, for the earlier piece.  An exact zero of f at a critical point is a root of that recursion, so a trajectory that
 * touches the plane without changing sides counts as a crossing, with NORMAL_SPEED 0.
 * At a crossing: p, v, a of the piece, h = a + g e3, zB = h / sqrt(h.h), yB = (0, zB.z, -zB.y) / sqrt(zB.z^2 + zB.y^2), xB = yB x zB (the frame of the
 * check and the penalty, with square root and division in place of their fast reciprocal root); d = p - c, s = eu.d, t = ev.d;
 *   ru = sqrt((e0 xB.eu)^2 + (e1 yB.eu)^2 + (e2 zB.eu)^2), rv likewise with ev: the body ellipsoid's reach along the gate's axes, in the form of
 *   FRX_CHECK_CORRIDOR, WITHOUT safe_margin;   MARGIN = min(wu - |s| - ru, wv - |t| - rv);   the crossing PASSES when MARGIN >= 0.
 * Fields of a gate's row (FRX_GATE_FIELDS doubles):
 *   FRX_GATE_N_CROSS, FRX_GATE_N_PASS   crossings and passing crossings over all the candidate's pieces (sums of integers: exact)
 *   the REPORTED crossing: FRX_GATE_MARGIN; FRX_GATE_TIME from the candidate's start, cum[k] + tau T_k with cum summed left to right as
 *   frx_trajectory_sample defines it; FRX_GATE_PIECE the local index k; FRX_GATE_U (s), FRX_GATE_V (t); FRX_GATE_REACH_U (ru), FRX_GATE_REACH_V (rv);
 *   FRX_GATE_NORMAL_SPEED n.v, signed
 * The reported crossing is the least under one total order: a crossing whose margin is NaN first, then passing crossings before the others; among
 * passing ones the earlier (piece, then root); among the others the larger margin, then the earlier.  So the row names the first passage if there is
 * one and the nearest miss otherwise.  No crossing: N_CROSS = N_PASS = 0, MARGIN = -inf, PIECE = -1, the other fields 0.  All ten fields NaN when a
 * piece of the candidate has T not finite or <= 0 or a coefficient not finite, or when the gate record is not finite or has |a|, |b| or |a x b|
 * equal to 0.  Rows are bit-identical run to run, between the forms, and whatever else is in the batch.  Flags per candidate: FRX_GATE_FLAG_*.
 * What the certificate is NOT.  It holds at the instant the body's centre is in the gate's plane.  The reach is the body's full projection on the
 * gate's axis, which is at least its section by the plane: conservative in extent.  It is not swept in time: a long body at a shallow angle may
 * touch the frame before or after that instant.  The gate's frame as an obstacle belongs to frx_trajectory_clearance.
 *   frx_gate_from_corners        host only, no device: n gates of four corners in order round the opening (corners n x 12, what
 *                                se3_node_cpu.cpp:44-61 reads) -> records (gates n x 9).  c = (((c0 + c1) + c2) + c3) / 4 (the reference's sum),
 *                                a = ((c1 - c0) + (c2 - c3)) / 4, b = ((c3 - c0) + (c2 - c1)) / 4.  fit (n x 2, may be NULL):
 *                                {a.b / (|a| |b|), max_i |corner_i - (c -/+ a -/+ b)|} - how far from a rectangle the corners are.
 *   frx_trajectory_gates         blocking, host pointers: T[total fine pieces], C[total fine pieces x 18], gate_off[B + 1], gates[gate_off[B] x 9];
 *                                gate_out (gate_off[B] x 10); flags (B) may be NULL and is filled as frx_gate_flags fills it.  Keeps one device buffer
 *                                per handle for the gates and grows it (FRX_ERR_ALLOC when it cannot).
 *   frx_trajectory_gates_device  ONE launch on the caller's stream, device pointers: no copy, no synchronisation, no allocation (capturable in a
 *                                hipGraph).  The caller vouches for gate_off_dev: monotone, starting at 0, ending at n_gates.
 *   frx_gate_flags               host only: the flag words from gate rows (for callers of the _device form).
 * FRX_ERR_INVALID_ARG, reported before a device is looked for: NULL arguments (flags of the blocking form and fit excepted), n or B < 1,
 * n_gates < 1 (device form), gate_off[0] != 0 or a non-monotone gate_off (frx_gate_flags).  FRX_ERR_NO_DEVICE without a device.  The blocking form
 * reads B from the handle - a handle exists only where a device does - and then returns FRX_ERR_INVALID_ARG for gate_off[0] != 0, a non-monotone
 * gate_off or gate_off[B] < 1, before anything is staged.  Serves both kinds of handle. */
#define FRX_GATE_FIELDS 10
#define FRX_GATE_N_CROSS 0
#define FRX_GATE_N_PASS 1
#define FRX_GATE_MARGIN 2
#define FRX_GATE_TIME 3
#define FRX_GATE_PIECE 4
#define FRX_GATE_U 5
#define FRX_GATE_V 6
#define FRX_GATE_REACH_U 7
#define FRX_GATE_REACH_V 8
#define FRX_GATE_NORMAL_SPEED 9
#define FRX_GATE_FLAG_MISSED 1u         /* a gate with N_PASS == 0 */
#define FRX_GATE_FLAG_REPEAT 2u         /* a gate with N_PASS > 1 */
#define FRX_GATE_FLAG_ORDER 4u          /* the TIMEs of the gates that passed are not strictly increasing in gate order */
#define FRX_GATE_FLAG_NONFINITE 8u      /* a NaN in one of the candidate's rows */
int frx_gate_from_corners(int n, const double *corners /* n x 12 */, double *gates /* n x 9 */, double *fit);
int frx_trajectory_gates(frx_problem *p, const double *T, const double *C, const int *gate_off /* B + 1 */, const double *gates,
                         double *gate_out /* gate_off[B] x FRX_GATE_FIELDS */, unsigned *flags /* B, may be NULL */);
int frx_trajectory_gates_device(frx_problem *p, const double *T_dev, const double *C_dev, int n_gates, const int *gate_off_dev,
                                const double *gates_dev, double *gate_out_dev, void *hip_stream);
int frx_gate_flags(int B, const int *gate_off, const double *gate_rows, unsigned *flags);

/* Exact corridor containment certificate of a batch of results, on the device.  frx_trajectory_check samples the corridor at M + 1 nodes per piece: a
 * body that pokes past a face between two nodes is reported as inside.  The reference never checks the corridor it optimises against at all.  These
 * entries decide, for every piece and every face of its polytope, at which instants the body ellipsoid touches the face and during which intervals it
 * is past it - nothing is sampled.
 * The body is E = diag(eh, eh, ev) (horiz_half_len twice, vert_half_len), the face normals are unit vectors and [xB yB zB] is orthonormal, so
 *   |E R^T n|^2 = eh^2 + Delta (zB.n)^2,   Delta = ev^2 - eh^2,   zB = h / |h|,   h = a + g e3.
 * With d(tau) = n.(p - p_k) + slack (quintic), Q = h.h (degree 6) and u = n.h (cubic) the signed reach sd = d + |E R^T n| is zero exactly where
 *   F(tau) = (d^2 - eh^2) Q - Delta u^2 = 0   and   d(tau) <= 0                                  (degree 16)
 * (a root of F with d > 0 belongs to the far side of the ellipsoid and is dropped).  slack pulls every face in by that much: 0 is the face of
 * FRX_CHECK_CORRIDOR, cfg.safe_margin the face the penalty aims at.  The roots are found as frx_trajectory_extrema finds roots (every sign change on
 * [0, 1] in normalised time, bracketed by the derivative's roots and bisected down to adjacent doubles).
 * Per face: a face with max d + max(eh, ev) < 0 is skipped (the body cannot reach it: no contact).  Otherwise the contacts in ascending order; an exact
 * root at tau == 0 is dropped unless the piece is its candidate's first (a knot on a contact counts once, for the earlier piece).  Each interval of
 * {0, contacts.., 1} is classed by sd at its midpoint with the direct formula; sd > 0, or a value that is not a number, is OUTSIDE.  The face's outside
 * time is the left-to-right sum of its outside intervals, times T.
 * Fields of a piece's row (FRX_CONTAIN_FIELDS doubles, times local in [0, T]):
 *   FRX_CONTAIN_N_CONTACT   contact instants, summed over the piece's faces (an exact integer)
 *   FRX_CONTAIN_OUTSIDE     the longest total time the body spends past one face, as a maximum over faces; 0: certified inside at every instant
 *   FRX_CONTAIN_T_EXIT, _T_ENTER, _K_EXIT   start and end of the earliest interval during which the body is past some face, and that face (the lowest
 *                           k on a tie); T_ENTER = T when the body is still out at the piece's end; all three -1 when there is no such interval
 *   FRX_CONTAIN_CENTRE, _T_CENTRE, _K_CENTRE   the exact maximum over faces and time of d, WITHOUT the reach, from the roots of the quartic d' and the
 *                           two ends (candidate order and ties as frx_trajectory_extrema; over faces the larger value, then the lower k).  It gives
 *                           the rigorous enclosure CENTRE + min(eh, ev) <= max sd <= CENTRE + max(eh, ev).
 * T not finite or <= 0, or a coefficient not finite: all eight NaN.  A row depends on its piece's own T, C, faces, g, eh, ev and slack and on whether
 * the piece is its candidate's first; rows are bit-identical run to run, between the forms, and whatever else is in the batch.
 * Candidate rows: N_CONTACT summed; OUTSIDE and CENTRE maxima in piece order (strict > replaces, a NaN takes the field and stays); the T_EXIT group
 * from the first piece that has one (or whose row is NaN); times from the candidate's start on the durations summed left to right; K_EXIT and
 * K_CENTRE hold the LOCAL PIECE index, as WORST_K's companion does in the check's candidate rows.  Flags: FRX_CHECK_FLAG_CORRIDOR when T_EXIT >= 0,
 * FRX_CHECK_FLAG_NONFINITE when a field of the candidate's row is not finite.
 * What the certificate is NOT.  The instants are exact, the depth of an excursion is not: CENTRE encloses max sd only to within |eh - ev|.  A contact
 * at which sd touches zero without changing sign may go uncounted (the intervals on both sides are classed the same, so OUTSIDE and T_EXIT are
 * unaffected).  h = 0 (free fall) leaves the attitude undefined: sd is not a number there and counts as outside.
 *   frx_trajectory_contain         blocking, host pointers (T[total fine pieces], C[total fine pieces x 18]); piece_out (pieces x 8) and flags (B)
 *                                  may be NULL, cand_out (B x 8) not.
 *   frx_trajectory_contain_device  ONE launch on the caller's stream, device pointers: no copy, no synchronisation, no allocation (capturable in a
 *                                  hipGraph); piece_out_dev (pieces x 8).
 *   frx_contain_fold               host only, no handle: candidate rows and flags from piece rows (for callers of the _device form); candidate b
 *                                  owns the pieces piece_off[b] .. piece_off[b + 1] - 1; cand_out and flags may each be NULL.
 *                                  A candidate without pieces leaves its row as it is and gets no flags.
 * FRX_ERR_INVALID_ARG, reported before a device is looked for: NULL arguments (the optional outputs excepted), a slack that is not finite, B < 1 or a
 * falling piece_off (frx_contain_fold).  FRX_ERR_NO_DEVICE without a device.  Serves both kinds of handle. */
#define FRX_CONTAIN_FIELDS 8
#define FRX_CONTAIN_N_CONTACT 0
#define FRX_CONTAIN_OUTSIDE 1
#define FRX_CONTAIN_T_EXIT 2
#define FRX_CONTAIN_T_ENTER 3
#define FRX_CONTAIN_K_EXIT 4
#define FRX_CONTAIN_CENTRE 5
#define FRX_CONTAIN_T_CENTRE 6
#define FRX_CONTAIN_K_CENTRE 7
int frx_trajectory_contain(frx_problem *p, const double *T, const double *C, double slack, double *piece_out, double *cand_out, unsigned *flags);
int frx_trajectory_contain_device(frx_problem *p, const double *T_dev, const double *C_dev, double slack, double *piece_out_dev, void *hip_stream);
int frx_contain_fold(int B, const int *piece_off, const double *T, const double *rows, double *cand_out, unsigned *flags);

/* Batched sampling of results with their SE(3) outputs, on the device.  The reference's traj_server evaluates one PolynomialTrajectory message at
 * control rate (traj_server.cpp:397-456: position, velocity, acceleration, jerk) and its controller derives attitude and thrust from the
 * acceleration; frx_msg_sample is that call for one time.  These entries sample every candidate of the handle's batch at S = n_samples times
 * each and write the flat state together with the flatness map the penalty and the check constrain (CPU.hpp:260-299).
 *   T, C        the batch's fine pieces as frx_optimize / frx_forward return them: T[P], C[P x 18], the handle's piece layout
 *   times       times != NULL: t = times[b S + s] (t0 and dt are not used)
 *               times == NULL, dt > 0: t_s = t0 + s dt;  dt == 0: t_s = s (total_b / (S - 1)), S >= 2 points over each candidate's duration
 *               Every time is measured from the candidate's own start.
 * Piece location: cum[0] = 0, cum[i + 1] = cum[i] + T[i] (left to right in piece order); t is clamped to [0, cum[N]]; the piece is the first i with
 * t <= cum[i + 1] (traj_server's `t > dur` rule: a knot time stays in the earlier piece); the local time is t - cum[i].  Past the end the state
 * of the end is held (traj_server extrapolates the last piece instead).  A NaN time gives a row of NaN.
 * Row of FRX_SAMPLE_FIELDS doubles, out[b][s][FRX_SAMPLE_FIELDS] row-major:
 *   FRX_SAMPLE_POS (3), FRX_SAMPLE_VEL (3), FRX_SAMPLE_ACC (3), FRX_SAMPLE_JERK (3)      p, v, a, j
 *   FRX_SAMPLE_THRUST     |h|, h = a + g e3 (collective thrust per unit mass)
 *   FRX_SAMPLE_QUAT (4)   (w, x, y, z) of R = [xB yB zB], zB = h / |h|, yB = normalise(0, zB.z, -zB.y), xB = yB x zB (the arithmetic of the check
 *                         and the penalty): Hamilton convention, R(q) = R maps body to world; the branch is taken on the largest of
 *                         (trace, R00, R11, R22), the earlier one on a tie, then the sign is chosen so that w >= 0
 *   FRX_SAMPLE_OMEGA (3)  body rates in the body frame: omega_x = -(yB.j) / |h|, omega_y = (xB.j) / |h|,
 *                         omega_z = -(xB.y dzB.z - xB.z dzB.y) / |(0, zB.z, -zB.y)| with dzB = (j - zB (zB.j)) / |h|;
 *                         |omega_xy| is the quantity the body-rate penalty and FRX_CHECK_BODY_RATE limit
 * There is no special case where h = 0 or zB.y = zB.z = 0: the arithmetic gives inf / NaN there, as in the penalty.  A non-finite T or C touches
 * its own candidate's rows only; rows are bit-identical run to run, between the two forms and whatever else is in the batch.
 *   frx_trajectory_sample         blocking, host pointers; keeps one device buffer per handle and grows it (FRX_ERR_ALLOC when it cannot).
 *   frx_trajectory_sample_device  a pure launch on the caller's stream, device pointers: no copy, no synchronisation, no allocation (capturable in
 *                                 a hipGraph); out_dev 16-byte aligned.
 * FRX_ERR_INVALID_ARG: n_samples < 1 (< 2 with times == NULL and dt == 0), dt < 0, t0 or dt not finite, T, C or out NULL, S x B x 20 overflowing
 * size_t.  Serves both kinds of handle (frx_problem_create[_from_h], frx_penalty_problem_create). */
#define FRX_SAMPLE_FIELDS 20
#define FRX_SAMPLE_POS 0
#define FRX_SAMPLE_VEL 3
#define FRX_SAMPLE_ACC 6
#define FRX_SAMPLE_JERK 9
#define FRX_SAMPLE_THRUST 12
#define FRX_SAMPLE_QUAT 13
#define FRX_SAMPLE_OMEGA 17
int frx_trajectory_sample(frx_problem *p, const double *T, const double *C, int n_samples, double t0, double dt, const double *times, double *out);
int frx_trajectory_sample_device(frx_problem *p, const double *T_dev, const double *C_dev, int n_samples, double t0, double dt,
                                 const double *times_dev, double *out_dev, void *hip_stream);

/* Clearance of a batch of results against the obstacle cloud itself, on the device.  frx_trajectory_check measures how far the body reaches past the
 * faces of corridors the library (or the caller) built; nothing there sees the point cloud the corridors came from, so a defect in corridor
 * generation, in the piece <-> polytope map or in a caller's own corridors is invisible to it.  The reference has no such test either
 * (MinCoPlan_CPU.cpp:131-132 prints getMaxVelRate / getMaxAccRate and flies).
 * Every fine piece is sampled at s_j = j (T / M), j = 0..M, M = intervals (1..FRX_CHECK_MAX_INTERVALS; the step is formed first, then multiplied,
 * as in the check).  At each sample: p and the frame R = [xB yB zB](h), h = a + g e3, in the check's arithmetic; E = diag(ellipsoid).  For every
 * cloud point o_i, i = 0..n_obs-1 (obs: n_obs x 3 doubles as frx_dilate_batch takes them):
 *   u = o_i - p (the difference is formed first);  q = (xB.u / e0)^2 + (yB.u / e1)^2 + (zB.u / e2)^2;  r = u.u
 * q is the square of decomp_util's Ellipsoid::dist for the body ellipsoid C = R E: q < 1 means the point is inside the body.
 * Fields of a row (FRX_CLEAR_FIELDS doubles):
 *   FRX_CLEAR_ELL       sqrt(min q), dimensionless; >= 1 means free (one IEEE square root of the minimum)
 *   FRX_CLEAR_DIST      sqrt(min r), metres from the body centre (its minimiser is not reported)
 *   FRX_CLEAR_WORST_T   local time s_j of the sample that attains min q
 *   FRX_CLEAR_WORST_I   index i of the cloud point that attains it
 * The worst (q, j, i) is taken under a total order: NaN beats any number, then the smaller q, then the lower j, then the lower i.  min r propagates
 * NaN.  A non-finite T, C or cloud point therefore shows as NaN and is never hidden by a minimum.  A candidate's row reduces its pieces in piece order
 * with the same order (an earlier piece before a later one); there WORST_T is the time from the candidate's start, the durations summed left to
 * right.  Flags per candidate: FRX_CLEAR_FLAG_*.  Rows are bit-identical run to run, between the forms, whatever else is in the batch and however the
 * cloud is split over workgroups.
 *   frx_trajectory_clearance            blocking, host pointers: T[total fine pieces], C[total fine pieces x 18], obs[n_obs x 3]; piece_out (P x 4)
 *                                       and flags (B) may be NULL, cand_out (B x 4) may not.  Keeps one device buffer per handle for the cloud and
 *                                       grows it (FRX_ERR_ALLOC when it cannot).
 *   frx_trajectory_clearance_workspace  bytes of scratch the device form needs: a function of (total fine pieces, intervals, n_obs) alone, never of
 *                                       the device.  0 when the cloud is not split (work_dev may then be NULL).
 *   frx_trajectory_clearance_device     pure launches on the caller's stream, device pointers: no copy, no synchronisation, no allocation
 *                                       (capturable in a hipGraph); piece rows only.
 * FRX_ERR_INVALID_ARG: n_obs < 1 or > FRX_CLEAR_MAX_POINTS, intervals out of range, NULL pointers.  Serves both kinds of handle
 * (frx_problem_create[_from_h], frx_penalty_problem_create). */
#define FRX_CLEAR_MAX_POINTS (1 << 24)
#define FRX_CLEAR_FIELDS 4
#define FRX_CLEAR_ELL 0
#define FRX_CLEAR_DIST 1
#define FRX_CLEAR_WORST_T 2
#define FRX_CLEAR_WORST_I 3
#define FRX_CLEAR_FLAG_COLLISION 1u     /* ELL < 1 */
#define FRX_CLEAR_FLAG_NONFINITE 2u     /* a non-finite value in the candidate's row */
int frx_trajectory_clearance(frx_problem *p, const double *T, const double *C, int intervals, int n_obs, const double *obs, double *piece_out,
                             double *cand_out, unsigned *flags);
int frx_trajectory_clearance_workspace(frx_problem *p, int intervals, int n_obs, size_t *bytes);
int frx_trajectory_clearance_device(frx_problem *p, const double *T_dev, const double *C_dev, int intervals, int n_obs, const double *obs_dev,
                                    void *work_dev, double *piece_out_dev, void *hip_stream);

/* Exact clearance certificate of a batch of results against the obstacle cloud, on the device.  frx_trajectory_clearance evaluates the body ellipsoid at
 * M + 1 instants a piece: a cloud point the body sweeps over between two samples is not seen, and a larger M costs P (M + 1) n_obs tests and still proves
 * nothing.  These entries find, for every piece, the exact minimum over time and over the cloud of the two quantities the dense form reports - nothing is
 * sampled.
 * The body is E = diag(eh, eh, ev) (horiz_half_len twice, vert_half_len) and [xB yB zB] is orthonormal, so for a cloud point o with u = o - p, h = a + g e3,
 * zB = h / |h| the squared ellipsoid distance is
 *   q = ((u.u) - (zB.u)^2) / eh^2 + (zB.u)^2 / ev^2,   r = u.u
 * which is the dense form's q with e0 = e1: the frame's x and y axes drop out, and with them the singularity where the dense frame's yB degenerates; q is
 * not a number only where h = 0.  In normalised time tau = t / T with w_k = c_k T^k and wh = T^2 (a + g e3), as frx_trajectory_contain forms them:
 * u = o - p(tau) is a quintic whose constant term is o - w_0 (the difference first), S = u.u has degree 10, Q = wh.wh degree 6, m = u.wh degree 8,
 *   r = S,   q = (S - m^2 / Q) / eh^2 + (m^2 / Q) / ev^2.
 * The minima of r over the piece lie among the roots of S' (degree 9) and the piece's ends; those of q among the roots of
 *   F = ev^2 S' Q^2 - (ev^2 - eh^2) m (2 m' Q - m Q')                                            (degree 21)
 * (Q^2 times the numerator of d/dtau [ev^2 S + (eh^2 - ev^2) m^2 / Q]) and the ends.  The roots are found as frx_trajectory_extrema finds roots (every
 * sign change on [0, 1], bracketed by the derivative's roots and bisected down to adjacent doubles).  Candidates: the roots ascending, then tau = 0, then
 * tau = 1.  The VALUES never come from the expanded polynomials: r and q are evaluated at each candidate directly from p and wh, so an error in a root
 * enters a minimum only to second order and every reported number is a value the trajectory attains.  A point's minimum follows the rule of
 * frx_trajectory_extrema (the first candidate wins a tie, a NaN takes the field and stays); a q that rounds below 0 is taken as 0.
 * Fields of a piece's row (FRX_CLEAR_EXACT_FIELDS doubles, times local in [0, T]):
 *   FRX_CLEAR_EXACT_ELL      sqrt(min q), dimensionless; >= 1 means free          FRX_CLEAR_EXACT_DIST     sqrt(min r), metres from the body centre
 *   FRX_CLEAR_EXACT_T_ELL    the local time tau T at which min q is attained       FRX_CLEAR_EXACT_I_ELL    the index i of the cloud point that attains it
 *   FRX_CLEAR_EXACT_T_DIST, FRX_CLEAR_EXACT_I_DIST   likewise for min r
 * Over the cloud each minimum is taken under a total order: NaN first, then the smaller value, then the lower i.  T not finite or <= 0, or a coefficient
 * not finite: all six NaN.  A cloud point that is not finite makes ELL NaN (DIST is NaN or +inf of that point) and is never hidden.
 * Most of the cloud is far from a piece, and the library leaves such points out by rules that are rigorous (fast-racing_amd/csrc/frx_clear_exact_kernel.hpp:
 * a lower bound from the box of the piece's Bezier control points against upper bounds that are values at candidates): they change the work, never a
 * row.  Rows are bit-identical run to run, between the forms, whatever else is in the batch and however the cloud is split over workgroups.
 * Candidate rows: each of the two minima with its time and point under the same order, an earlier piece before a later one; times from the candidate's
 * start on the durations summed left to right.  Flags: FRX_CLEAR_FLAG_COLLISION (ELL < 1), FRX_CLEAR_FLAG_NONFINITE.
 * What the certificate is NOT.  The instants are exact to the root finder's bisection (adjacent doubles of tau where the critical polynomial changes
 * sign); a critical point at which the polynomial touches zero without changing sign is no candidate, which can only miss a point of inflection, never
 * a minimum.  h = 0 (free fall) leaves the attitude undefined: q is not a number at such an instant and ELL reports it.
 *   frx_trajectory_clearance_exact            blocking, host pointers: T[total fine pieces], C[total fine pieces x 18], obs[n_obs x 3]; piece_out (P x 6)
 *                                             and flags (B) may be NULL, cand_out (B x 6) may not.  Uses the handle's cloud buffer as the dense form does
 *                                             and grows it (FRX_ERR_ALLOC when it cannot).
 *   frx_trajectory_clearance_exact_workspace  bytes of scratch the device form needs: a function of (total fine pieces, n_obs) alone, never of the device;
 *                                             never 0.
 *   frx_trajectory_clearance_exact_device     pure launches on the caller's stream, device pointers: no copy, no synchronisation, no allocation (capturable
 *                                             in a hipGraph); piece rows only.
 *   frx_clearance_exact_fold                  host only, no handle: candidate rows and flags from piece rows (for callers of the _device form); candidate b
 *                                             owns the pieces piece_off[b] .. piece_off[b + 1] - 1; cand_out and flags may each be NULL.
 * FRX_ERR_INVALID_ARG, reported before a device is looked for: NULL pointers (the optional outputs excepted), n_obs < 1 or > FRX_CLEAR_MAX_POINTS, B < 1
 * or a falling piece_off (frx_clearance_exact_fold).  FRX_ERR_NO_DEVICE without a device.  Serves both kinds of handle. */
#define FRX_CLEAR_EXACT_FIELDS 6
#define FRX_CLEAR_EXACT_ELL 0
#define FRX_CLEAR_EXACT_DIST 1
#define FRX_CLEAR_EXACT_T_ELL 2
#define FRX_CLEAR_EXACT_I_ELL 3
#define FRX_CLEAR_EXACT_T_DIST 4
#define FRX_CLEAR_EXACT_I_DIST 5
int frx_trajectory_clearance_exact(frx_problem *p, const double *T, const double *C, int n_obs, const double *obs, double *piece_out, double *cand_out,
                                   unsigned *flags);
int frx_trajectory_clearance_exact_workspace(frx_problem *p, int n_obs, size_t *bytes);
int frx_trajectory_clearance_exact_device(frx_problem *p, const double *T_dev, const double *C_dev, int n_obs, const double *obs_dev, void *work_dev,
                                          double *piece_out_dev, void *hip_stream);
int frx_clearance_exact_fold(int B, const int *piece_off, const double *T, const double *rows, double *cand_out, unsigned *flags);

/* A batch of results screened against a field over the voxel map's grid, on the device: P (M + 1) look-ups that tell a caller which pieces of which
 * candidates are worth frx_trajectory_clearance or frx_trajectory_clearance_exact - both take any (T, C) batch, so only the doubtful pieces need go there.
 * field is any double array over map's grid, x fastest: pos or all of frx_map_esdf (what MapUtil::getDistance reads, map_util.h:309-318), or a caller's own.
 * Every fine piece is sampled at s_j = j (T / M), j = 0..M, M = intervals (1..FRX_CHECK_MAX_INTERVALS; the step is formed first, then multiplied, as in the
 * check and the clearance).  The sample's cell is map_blocked's: round((p - origin) / res - 0.5) per axis, none of it fused.  A sample outside the map - a
 * position that is not a number included - is counted and left out of the minimum (the reference reads out of bounds there).
 * Fields of a piece's row (FRX_MAPDIST_FIELDS doubles):
 *   FRX_MAPDIST_DIST        the smallest field[cell] over the samples inside the map under the order: not a number first, then the smaller value, then the lower j
 *   FRX_MAPDIST_WORST_T     s_j of that sample
 *   FRX_MAPDIST_WORST_CELL  its linear cell index, as a double
 *   FRX_MAPDIST_OUTSIDE     the number of samples outside the map
 * A piece with no sample inside: DIST = +inf, WORST_T = WORST_CELL = -1.  A candidate's row keeps that order on (DIST, piece) - an earlier piece before a later
 * one - with WORST_T counted from the candidate's start on the durations summed left to right (-1 stays -1) and OUTSIDE summed.  Flags per candidate:
 * FRX_MAPDIST_FLAG_BELOW (DIST < margin), _OUTSIDE (OUTSIDE > 0), _NONFINITE (a field of the row is not finite: DIST = +inf among them); a candidate
 * without pieces keeps its row and gets no flag.  Rows are bit-identical run to run, between the forms and whatever else is in the batch.
 *   frx_trajectory_map_distance         blocking, host pointers: T[total fine pieces], C[total fine pieces x 18], field[cells]; piece_out (P x 4) and flags (B)
 *                                       may be NULL, cand_out (B x 4) may not.  Keeps one device buffer per handle for the field and grows it.
 *   frx_trajectory_map_distance_device  one launch on the caller's stream, device pointers: no copy, no synchronisation, no allocation (capturable); piece rows only.
 *   frx_map_distance_fold               host only, no handle: candidate rows and flags from piece rows; candidate b owns the pieces piece_off[b] ..
 *                                       piece_off[b + 1] - 1; cand_out and flags may each be NULL.
 * FRX_ERR_INVALID_ARG, reported before a device is looked for: NULL pointers (the optional outputs excepted; map->cells is not read), intervals out of range,
 * res not above 0, a dim <= 0, more than 2^31 - 1 cells, a margin that is not a number, B < 1 or a falling piece_off (the fold).  Serves both kinds of handle. */
#define FRX_MAPDIST_FIELDS 4
#define FRX_MAPDIST_DIST 0
#define FRX_MAPDIST_WORST_T 1
#define FRX_MAPDIST_WORST_CELL 2
#define FRX_MAPDIST_OUTSIDE 3
#define FRX_MAPDIST_FLAG_BELOW 1u
#define FRX_MAPDIST_FLAG_OUTSIDE 2u
#define FRX_MAPDIST_FLAG_NONFINITE 4u
int frx_trajectory_map_distance(frx_problem *p, const double *T, const double *C, int intervals, const frx_voxel_map *map, const double *field, double margin,
                                double *piece_out, double *cand_out, unsigned *flags);
int frx_trajectory_map_distance_device(frx_problem *p, const double *T_dev, const double *C_dev, int intervals, const frx_voxel_map *map, const double *field_dev,
                                       double *piece_out_dev, void *hip_stream);
int frx_map_distance_fold(int B, const int *piece_off, const double *T, const double *rows, double margin, double *cand_out, unsigned *flags);

/* Replaces ~cuda_computer / kill_kernel (cc.cu:44-49, 566-579; GPU.hpp:907-909). */
void frx_problem_destroy(frx_problem *p);

/* Where the O(n) state of L-BFGS lives during frx_optimize.  In both modes every decision (Moré–Thuente / backtracking
 * line search, convergence and stop tests, error codes: lbfgs.hpp:730-1033, 1295-1352) is taken on the host.
 *   FRX_LBFGS_DEVICE_VECTORS (default) x, g, d, the (s,y) history and the two-loop recursion (lbfgs.hpp:1354-1411) stay on the
 *                            device; per round and candidate 32 B of command go down and 40 B of scalars come back.
 *   FRX_LBFGS_HOST_VECTORS   the vectors live on the host and run in the reference's exact operation order (bit-identical
 *                            iterates given identical f, g); the gradient crosses PCIe every round.
 * The environment variable FRX_LBFGS=host|device overrides the default. */
#define FRX_LBFGS_DEVICE_VECTORS 0
#define FRX_LBFGS_HOST_VECTORS 1
int frx_problem_set_lbfgs_mode(frx_problem *p, int mode);

/* How the MINCO map (q,T)->c and its adjoint are evaluated on the device.  Both compute the same spline:
 *   FRX_SOLVER_KNOT_PCR  (default) quintic-Hermite knot form, SPD 2x2-block tridiagonal system in the knot (v,a),
 *                        parallel cyclic reduction: O(log N) depth (fast-racing_amd/csrc/frx_minco.hpp)
 *   FRX_SOLVER_BANDED_LU the reference's own elimination order: 6N x 6N band, no-pivot LU, solve, solveAdj
 *                        (trajectory.hpp:655-751); sequential in 6N, kept as an on-device cross-check. */
#define FRX_SOLVER_KNOT_PCR 0
#define FRX_SOLVER_BANDED_LU 1
int frx_problem_set_solver(frx_problem *p, int solver);

/* Totals: out6 = {B, total fine pieces, total coarse pieces, total free variables, max half-spaces per piece,
 * sum over fine pieces of their half-space count}. */
int frx_problem_totals(const frx_problem *p, int *out6);
/* Offsets (each B+1 ints): fine pieces, coarse pieces, free variables; plus dimFreeT per candidate (B ints).
 * Candidate b's variables are x[x_off[b] .. x_off[b+1]) = (tau[dim_t[b]], xi[...]) as in CPU.hpp:970-971. */
int frx_problem_layout(const frx_problem *p, int *piece_off, int *coarse_off, int *x_off, int *dim_t);

/* First half of SE3GCOPTER::optimize (CPU.hpp:1237-1240): setInitial + backwardT + backwardP.
 * Host work (tiny NLS solves, CPU.hpp:777-813); x0 has total-free-variables doubles. */
int frx_initial_guess(frx_problem *p, double *x0);

/*
 * Replaces SE3GCOPTER::objectiveFunc (CPU.hpp:961-1000) for the whole batch: x -> (f, grad).
 * One call = steps 1-7 of SURVEY.md §3.4 for every candidate, entirely on the device.
 *   x, g : total-free-variables doubles;  f : B doubles.
 * On the device this is ONE kernel launch (clusters of workgroups, one per candidate) when every candidate has <= 64 pieces and the chip holds the whole batch at
 * once, three stage launches otherwise; the _device form is a pure sequence of launches on the caller's stream (capturable in a hipGraph), one evaluation in flight
 * per handle.  Should a wait inside the one-launch form expire (a device shared with other grids: INTEGRATION.md 8) the objective values concerned are NaN and the
 * blocking form returns FRX_ERR_TIMEOUT; the handle then continues with the three launches.
 */
int frx_objective_eval(frx_problem *p, const double *x, double *f, double *g);
int frx_objective_eval_device(frx_problem *p, const double *x_dev, double *f_dev, double *g_dev, void *hip_stream);
/* The _device form has no host-synchronous point of its own.  After the caller has synchronised its stream: FRX_OK, or FRX_ERR_TIMEOUT when a wait inside a
 * one-launch evaluation expired since the last check (objective values NaN from that evaluation on; the word is cleared and the handle continues with three
 * launches per evaluation).  Direct calls notice by themselves - the first frx_objective_eval_device after the failure became visible takes the three launches -
 * but a captured hipGraph replays what was captured: a caller that replays graphs polls this (or the NaN objective values). */
int frx_eval_status(frx_problem *p);

/*
 * Replaces cuda_computer::compute (cc.cuh:118-134, cc.cu:469-563) = MINCO_S3::addTimeIntPenalty
 * (CPU.hpp:188-408) for the whole batch, with the same ACCUMULATING semantics (cc.cu:551-558):
 *   cost[b] += penalty,  gdT[piece] += d/dT,  gdC[piece*18 ..] += d/dc.
 *   T    : total-fine-pieces doubles (piece durations)
 *   C    : total-fine-pieces x 18 doubles (piece-major coefficients)
 * The _device variant OVERWRITES per-piece partials out_dev[piece*20 + {0: cost, 1: gdT, 2..19: gdC}]
 * and leaves the accumulation to the caller.
 */
int frx_penalty_eval(frx_problem *p, const double *T, const double *C, double *cost, double *gdT, double *gdC);
int frx_penalty_eval_device(frx_problem *p, const double *T_dev, const double *C_dev, double *out_dev, void *hip_stream);
/*
 * The inner boundary ON ITS OWN: a handle built from exactly what cuda_computer::compute receives on every call (cc.cuh:118-134, call site GPU.hpp:219-227) -
 * idxHs, cfgHs, ellipsoid, safeMargin, the limits, the weights ci, cons = cfg->qd_intervals for every piece (GPU.hpp:963-964) - for a caller that keeps the
 * reference's MINCO_S3 / SE3GCOPTER on the host and swaps only `class cuda_computer` (oracle/frx_dropin/cuda_computer.cuh is that class; the reference's
 * se3gcopter_gpu.hpp compiles against it unmodified, tests/test_reference_gpu_header.py).  Polytopes and parameters go up ONCE here instead of through mapped
 * memory on every call (cc.cu:492-527).
 *   piece_n[B]             pieces per candidate
 *   piece_poly[sum pieces] index m of every piece's polytope in the CSR below (= idxHs)
 *   h_off, h_rec           CSR of the H-polytopes, 6 doubles per half-space (outer normal, point) = one column of cfgHs[m]
 * Such a handle serves frx_penalty_eval and frx_penalty_eval_device; every entry point that needs variables or waypoint polytopes returns FRX_ERR_INVALID_ARG.
 */
int frx_penalty_problem_create(const frx_config *cfg, int device, int B, const int *piece_n, const int *piece_poly,
                               const int *h_off, const double *h_rec, frx_problem **out);

/* x -> piece durations T (total fine pieces) and coefficients C (x 18): forwardT/forwardP + MINCO_S3::generate
 * (CPU.hpp:1258-1262, 425-505).  Either output may be NULL. */
int frx_forward(frx_problem *p, const double *x, double *T, double *C);

/*
 * Replaces SE3GCOPTER::optimize (CPU.hpp:1230-1268) for the whole batch: every candidate runs
 * its own L-BFGS (host, lbfgs.hpp:1103-1444 semantics incl. the Moré–Thuente search and the
 * backtracking fallback); all candidates that need an objective value at a given moment share
 * ONE batched device evaluation.
 *   x        in: start point (from frx_initial_guess or the caller); out: minimiser
 *   C, T     optimised coefficients / durations of the final generate() (CPU.hpp:1262-1263); may be NULL
 *   jerk_cost[B]   what the reference returns (CPU.hpp:1267); may be NULL
 *   objective[B]   final penalised objective (discarded by the reference, CPU.hpp:1242); may be NULL
 *   status[B]      lbfgs_optimize return code per candidate (ignored by the reference, CPU.hpp:1249)
 *   iters[B], evals[B]  iteration / evaluation counts; may be NULL
 */
int frx_optimize(frx_problem *p, const frx_lbfgs_params *params, double *x, double *C, double *T,
                 double *jerk_cost, double *objective, int *status, int *iters, int *evals);

/* Wall-clock split of the last frx_optimize call, milliseconds: out4 = {total, device evaluations
 * (launch + copies + sync), host L-BFGS, evaluation rounds}. */
int frx_optimize_stats(const frx_problem *p, double *out4);

/*
 * How frx_optimize runs a plan on the device.  The reference's device side is ONE kernel that stays resident and is driven through
 * a mailbox in mapped host memory (cc.cu:51-64, 396-405, 454-466, 535-548); the default here has the same shape: the RESIDENT ROUND
 * KERNEL (csrc/frx_round_kernel.hpp) - one launch per plan, a cluster of workgroups per candidate, history of the L-BFGS in
 * registers, per-cluster command/result mailboxes - whenever the batch fits the chip (B x G workgroups <= CUs, mem_size <= 128).
 * A batch of up to a few times that many candidates runs on the same kernel through a WORK QUEUE: as many clusters as the chip holds
 * stay resident, and a cluster whose candidate is finished is handed the next one of the batch instead of leaving.  Still larger
 * batches, and any launch on which a device-side wait expires, run one launch per stage and round (k_lbfgs_pre -> k_forward_knot ->
 * k_penalty -> k_backward_knot) - the faster form for many hundreds of candidates.  frx_problem_set_resident(p, 0) pins a handle to
 * the per-stage rounds (environment: FRX_RESIDENT=0), 1 is the default just described, 2 takes the work queue for every batch that
 * exceeds the chip (environment: FRX_RESIDENT_QUEUE=0|1 forbids / forces the queue).  frx_optimize_path reports what the last plan used
 * (0 = per-stage rounds, G > 0 = resident kernel with G workgroups per candidate) and the resident kernel's device-side status word
 * (0 = clean; otherwise the code of the wait that expired).
 */
int frx_problem_set_resident(frx_problem *p, int enable);
int frx_optimize_path(const frx_problem *p, int *resident_used, unsigned *device_status);
/*
 * Multi-GPU plans (the reference is pinned to device 0, cc.cu:414).  The batch is block-partitioned over the devices:
 * one host thread + one frx_problem handle per device runs its shard exactly like frx_optimize - candidates are independent, an
 * evaluation needs no collective - and the plan ends with the winner exchange over RCCL (ncclCommInitAll over the devices of this
 * process): all-gather of (objective, candidate id), 16 bytes per device, then a broadcast of the winner's 6N x 3 coefficients and
 * N durations from the device that owns it.  librccl.so is loaded on first use.  n_devices = 0 takes every visible device (never
 * more shards than candidates); `devices` may be NULL (0, 1, ...).  When several shards share a physical device (tests on a 1-GPU
 * box; RCCL refuses duplicates), or with FRX_MULTI_COMM=host, the same two operations run through an in-process communicator.
 * Arrays of frx_multi_optimize are packed over the WHOLE batch in candidate order (offsets: frx_multi_layout); C, T, jerk_cost,
 * objective, iters, evals and the winner_* outputs may be NULL.  Failed candidates (status < 0) and non-finite objectives never win,
 * ties go to the lowest id; winner_C / winner_T hold winner_n pieces (18 doubles each / one duration each).
 */
typedef struct frx_multi frx_multi;
int frx_multi_create(const frx_config *cfg, int n_devices, const int *devices, int B, const int *coarse_n, const double *ini_state,
                     const double *fin_state, const int *h_off, const double *h_rec, const int *v_off, const double *v_rec, frx_multi **out);
void frx_multi_destroy(frx_multi *m);
int frx_multi_info(const frx_multi *m, int *n_shards, int *uses_rccl, int *shard_lo, int *shard_device);
int frx_multi_layout(const frx_multi *m, int *piece_off, int *x_off);
int frx_multi_initial_guess(frx_multi *m, double *x0);
int frx_multi_optimize(frx_multi *m, const frx_lbfgs_params *params, double *x, double *C, double *T, double *jerk_cost, double *objective,
                       int *status, int *iters, int *evals, int *winner_id, double *winner_objective, double *winner_C, double *winner_T,
                       int *winner_n);
/* 1 when the last frx_multi_optimize exchanged the winner through RCCL, 0 for the in-process communicator. */
int frx_multi_last_exchange(const frx_multi *m);

/*
 * Host-side solver on its own (used by the CPU tests and by integrators that bring their own
 * objective): minimises `count` independent problems with the batched state machine.  `eval`
 * is called with the ids of the problems that need a value; x/g are the packed arrays
 * (problem i at x_off[i]).  Semantics of each problem = lbfgs::lbfgs_optimize (lbfgs.hpp:1103).
 */
typedef void (*frx_batch_eval_fn)(void *instance, int n_active, const int *active_ids,
                                  const double *x, double *f, double *g);
int frx_lbfgs_minimize_batch(int count, const int *x_off, double *x, double *f_out, int *status, int *iters, int *evals,
                             const frx_lbfgs_params *params, frx_batch_eval_fn eval, void *instance, int n_threads);

#ifdef __cplusplus
}
#endif
#endif /* FRX_H */
