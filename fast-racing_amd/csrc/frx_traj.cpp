// The trajectory entries of the C ABI: what is asked of pieces (T, C) a handle's candidates lay out - check, extrema, gates, contain, clearance, exact clearance,
// map distance and sample - with their workspace queries, the handle-less folds and the tests' switches.  They have one shape.  A DEVICE form takes device
// pointers and a stream, checks its arguments and only launches (nothing is allocated, copied or waited for: it can be captured in a graph).  A BLOCKING form
// takes host buffers: it sets the handle's device, grows the scratch buffer it carves up (frx_traj_host.hpp), stage_TC ((T, C) -> d_T, d_C through the pinned
// h_T, h_C), its own operands, the device form on the handle's stream, fetch_rows, then - where there are piece rows - the fold to candidate rows and flag words
// on the host (frx_traj_fold.hpp, frx_gate_host.hpp).  What an entry decides on the host is in frx_traj_host.hpp, where tests/hostcheck reaches it without a
// device.  Verdicts come in one order: null arguments, the rules of the scalars and offsets, "no HIP device" (the check and the dense clearance do not look for
// one), then whatever reads the handle: capacity, allocation, HIP errors.
#include <hip/hip_runtime_api.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/frx.h"
#include "../../include/frx_debug.h"
#include "frx_handle.hpp"
#include "frx_batch_host.hpp"
#include "frx_gate_host.hpp"
#include "frx_traj_fold.hpp"
#include "frx_traj_host.hpp"

static_assert(FRX_EXTREMA_FIELDS == (int)frx::EXTREMA_FIELDS && FRX_GATE_FIELDS == (int)frx::GATE_FIELDS && FRX_CONTAIN_FIELDS == (int)frx::CONTAIN_FIELDS &&
              FRX_CLEAR_EXACT_FIELDS == (int)frx::CLEAR_EXACT_FIELDS && FRX_MAPDIST_FIELDS == (int)frx::MAPDIST_FIELDS, "frx.h and frx_device.hpp agree on the rows");
static_assert(FRX_CHECK_FIELDS <= 20 && FRX_EXTREMA_FIELDS <= 20 && FRX_CONTAIN_FIELDS <= 20 && FRX_CLEAR_FIELDS <= 20 && FRX_CLEAR_EXACT_FIELDS <= 20 && FRX_MAPDIST_FIELDS <= 20,
              "every row of pieces fits the P x 20 staging (h_out20, d_rows)");

namespace {

// the piece rows of the blocking check, extrema and contain: one [P][20] buffer, allocated by whichever runs first (each synchronises before it returns)
int piece_rows(frx_problem *p) {
    if (!p->d_rows.p) HIP_TRY(p->d_rows.alloc(20 * (size_t)p->P));
    return FRX_OK;
}

// what every form of frx_trajectory_clearance shares behind its null test: the scalars, then - reading the handle - the split of the cloud
int clear_split(frx_problem *p, int intervals, int n_obs, int *chunk, int *nchunks) {
    FRX_TRY(frx::intervals_arg(intervals));
    FRX_TRY(frx::cloud_points_arg(n_obs));
    if (!frx::cloud_split(p->P, n_obs, p->clear_chunk, frx::CLEAR_PASS, frx::CLEAR_TARGET_WGS, chunk, nchunks))
        return fail(FRX_ERR_CAPACITY, "frx_trajectory_clearance: " + std::to_string(p->P) + " pieces x the cloud's chunks exceed a grid");
    return FRX_OK;
}
size_t clear_work(const frx_problem *p, int nchunks) { return nchunks > 1 ? (size_t)FRX_CLEAR_FIELDS * p->P * (size_t)nchunks : 0; }   // one chunk: the kernel writes the rows itself

// likewise frx_trajectory_clearance_exact, which looks for a device in between
int clear_exact_split(frx_problem *p, int n_obs, int *chunk, int *nchunks) {
    FRX_TRY(frx::cloud_points_arg(n_obs));
    if (frx_device_count() < 1) return frx::no_device();
    if (!frx::cloud_split(p->P, n_obs, p->clx_chunk, frx::CLEAR_EXACT_CHUNK, frx::CLEAR_EXACT_TARGET_WGS, chunk, nchunks))
        return fail(FRX_ERR_CAPACITY, "frx_trajectory_clearance_exact: " + std::to_string(p->P) + " pieces x the cloud's chunks exceed a grid");
    return FRX_OK;
}
size_t clear_exact_work(const frx_problem *p, int nchunks) { return (size_t)frx::CLEAR_EXACT_PARTIAL * p->P * (size_t)nchunks; }

// what both forms of frx_trajectory_map_distance share behind their null test
int map_distance_args(int intervals, const frx_voxel_map *map) {
    FRX_TRY(frx::intervals_arg(intervals));
    FRX_TRY(frx::voxel_map_args(map, "frx_trajectory_map_distance", false));
    if (frx_device_count() < 1) return frx::no_device();
    return FRX_OK;
}

// what both forms of frx_trajectory_sample share behind their null test; *n_out = B x S x FRX_SAMPLE_FIELDS
int sample_args(frx_problem *p, int n_samples, double t0, double dt, bool have_times, size_t *n_out) {
    FRX_TRY(frx::sample_time_args(n_samples, t0, dt, have_times));
    FRX_TRY(frx::sample_rows_arg(p->B, n_samples, n_out));
    if (!frx::sample_fits(p->maxN)) return fail(FRX_ERR_CAPACITY, "frx_trajectory_sample: the prefix sums of " + std::to_string(p->maxN) + " pieces exceed the kernel's LDS");
    return FRX_OK;
}

// the null test of a handle-less fold, in its name
int fold_args(const char *who, int B, const int *piece_off, const double *T, const double *rows) {
    if (B < 1 || !piece_off || !T || !rows) return fail(FRX_ERR_INVALID_ARG, std::string(who) + ": B must be >= 1 and piece_off, T, rows not NULL");
    return FRX_OK;
}

} // namespace

extern "C" {

// ---- check ----
int frx_trajectory_check_device(frx_problem *p, const double *T_dev, const double *C_dev, int intervals, double *piece_out_dev, void *hip_stream) {
    if (!p || !T_dev || !C_dev || !piece_out_dev) return fail(FRX_ERR_INVALID_ARG, "null argument");
    FRX_TRY(frx::intervals_arg(intervals));
    int lpp = 0, ppw = 0;
    if (!frx::check_geometry(intervals, p->Kmax, &lpp, &ppw)) return fail(FRX_ERR_CAPACITY, "frx_trajectory_check: a corridor block of " + std::to_string(p->Kmax) + " half-spaces exceeds a wave's LDS");
    HIP_TRY((hipError_t)frx::launch_check(p->dp, p->Kmax, T_dev, C_dev, intervals, piece_out_dev, hip_stream));
    return FRX_OK;
}

int frx_trajectory_check(frx_problem *p, const double *T, const double *C, int intervals, double *piece_out, double *cand_out, unsigned *flags) {
    if (!p || !T || !C || !cand_out) return fail(FRX_ERR_INVALID_ARG, "null argument");
    FRX_TRY(frx::intervals_arg(intervals));
    HIP_TRY(hipSetDevice(p->device));
    FRX_TRY(piece_rows(p));
    FRX_TRY(stage_TC(p, T, C));
    FRX_TRY(frx_trajectory_check_device(p, p->d_T.p, p->d_C.p, intervals, p->d_rows.p, p->stream));
    FRX_TRY(fetch_rows(p, p->d_rows.p, (size_t)FRX_CHECK_FIELDS * p->P, piece_out));
    const double lim[4] = {p->cfg.vel_max, p->cfg.thr_acc_min, p->cfg.thr_acc_max, p->cfg.body_rate_max};
    frx::fold_check(p->B, p->poff.data(), T, p->h_out20.p, lim, cand_out, flags);
    return FRX_OK;
}

// ---- extrema ----
int frx_trajectory_extrema_device(frx_problem *p, const double *T_dev, const double *C_dev, double *piece_out_dev, void *hip_stream) {
    if (!p || !T_dev || !C_dev || !piece_out_dev) return fail(FRX_ERR_INVALID_ARG, "null argument");
    if (frx_device_count() < 1) return frx::no_device();
    HIP_TRY((hipError_t)frx::launch_extrema(p->P, p->dp.pc.gAcc, T_dev, C_dev, piece_out_dev, hip_stream));
    return FRX_OK;
}

int frx_trajectory_extrema(frx_problem *p, const double *T, const double *C, double *piece_out, double *cand_out, unsigned *flags) {
    if (!p || !T || !C || !cand_out) return fail(FRX_ERR_INVALID_ARG, "null argument");
    if (frx_device_count() < 1) return frx::no_device();
    HIP_TRY(hipSetDevice(p->device));
    FRX_TRY(piece_rows(p));
    FRX_TRY(stage_TC(p, T, C));
    FRX_TRY(frx_trajectory_extrema_device(p, p->d_T.p, p->d_C.p, p->d_rows.p, p->stream));
    FRX_TRY(fetch_rows(p, p->d_rows.p, (size_t)FRX_EXTREMA_FIELDS * p->P, piece_out));
    const double lim[4] = {p->cfg.vel_max, p->cfg.thr_acc_min, p->cfg.thr_acc_max, p->cfg.body_rate_max};
    frx::fold_extrema(p->B, p->poff.data(), T, p->h_out20.p, lim, cand_out, flags);
    return FRX_OK;
}

// ---- gates ----
int frx_gate_from_corners(int n, const double *corners, double *gates, double *fit) {
    if (n < 1 || !corners || !gates) return fail(FRX_ERR_INVALID_ARG, "frx_gate_from_corners: n must be >= 1 and corners, gates not NULL");
    frx::gate_from_corners(n, corners, gates, fit);
    return FRX_OK;
}

int frx_gate_flags(int B, const int *gate_off, const double *gate_rows, unsigned *flags) {
    if (B < 1 || !gate_off || !gate_rows || !flags) return fail(FRX_ERR_INVALID_ARG, "frx_gate_flags: B must be >= 1 and no argument NULL");
    FRX_TRY(frx::offsets_args("gate_off", B, gate_off, true));
    frx::gate_flags(B, gate_off, gate_rows, flags);
    return FRX_OK;
}

int frx_trajectory_gates_device(frx_problem *p, const double *T_dev, const double *C_dev, int n_gates, const int *gate_off_dev, const double *gates_dev,
                                double *gate_out_dev, void *hip_stream) {
    if (!p || !T_dev || !C_dev || !gate_off_dev || !gates_dev || !gate_out_dev) return fail(FRX_ERR_INVALID_ARG, "null argument");
    if (n_gates < 1) return fail(FRX_ERR_INVALID_ARG, "n_gates must be >= 1");
    if (frx_device_count() < 1) return frx::no_device();
    HIP_TRY((hipError_t)frx::launch_gates(p->B, p->dp.poff, p->dp.pc.gAcc, p->dp.pc.ell, T_dev, C_dev, n_gates, gate_off_dev, gates_dev, gate_out_dev, hip_stream));
    return FRX_OK;
}

int frx_trajectory_gates(frx_problem *p, const double *T, const double *C, const int *gate_off, const double *gates, double *gate_out, unsigned *flags) {
    if (!p || !T || !C || !gate_off || !gates || !gate_out) return fail(FRX_ERR_INVALID_ARG, "null argument");
    if (frx_device_count() < 1) return frx::no_device();
    FRX_TRY(frx::offsets_args("gate_off", p->B, gate_off, true));
    const int n_gates = gate_off[p->B];
    if (n_gates < 1) return fail(FRX_ERR_INVALID_ARG, "frx_trajectory_gates: no gates (gate_off[B] < 1)");
    HIP_TRY(hipSetDevice(p->device));
    const frx::Carve at = frx::carve_gates(n_gates, p->B);
    FRX_TRY(grow(p->d_gates, at.total, "frx_trajectory_gates"));
    double *d_rows = p->d_gates.p, *d_rec = d_rows + at.second;
    int *d_off = (int *)(d_rows + at.third);
    FRX_TRY(stage_TC(p, T, C));
    HIP_TRY(hipMemcpyAsync(d_rec, gates, sizeof(double) * (at.third - at.second), hipMemcpyHostToDevice, p->stream));
    HIP_TRY(hipMemcpyAsync(d_off, gate_off, sizeof(int) * ((size_t)p->B + 1), hipMemcpyHostToDevice, p->stream));
    FRX_TRY(frx_trajectory_gates_device(p, p->d_T.p, p->d_C.p, n_gates, d_off, d_rec, d_rows, p->stream));
    HIP_TRY(hipMemcpyAsync(gate_out, d_rows, sizeof(double) * at.second, hipMemcpyDeviceToHost, p->stream));   // (rows per gate, not per piece: no staging)
    HIP_TRY(hipStreamSynchronize(p->stream));
    if (flags) frx::gate_flags(p->B, gate_off, gate_out, flags);
    return FRX_OK;
}

// ---- contain ----
int frx_contain_fold(int B, const int *piece_off, const double *T, const double *rows, double *cand_out, unsigned *flags) {
    FRX_TRY(fold_args("frx_contain_fold", B, piece_off, T, rows));
    FRX_TRY(frx::offsets_args("frx_contain_fold: piece_off", B, piece_off, false));
    frx::fold_contain(B, piece_off, T, rows, cand_out, flags);
    return FRX_OK;
}

int frx_trajectory_contain_device(frx_problem *p, const double *T_dev, const double *C_dev, double slack, double *piece_out_dev, void *hip_stream) {
    if (!p || !T_dev || !C_dev || !piece_out_dev) return fail(FRX_ERR_INVALID_ARG, "null argument");
    if (!std::isfinite(slack)) return fail(FRX_ERR_INVALID_ARG, "slack must be finite");
    if (frx_device_count() < 1) return frx::no_device();
    HIP_TRY((hipError_t)frx::launch_contain(p->dp, p->Kmax, slack, T_dev, C_dev, piece_out_dev, hip_stream));
    return FRX_OK;
}

int frx_trajectory_contain(frx_problem *p, const double *T, const double *C, double slack, double *piece_out, double *cand_out, unsigned *flags) {
    if (!p || !T || !C || !cand_out) return fail(FRX_ERR_INVALID_ARG, "null argument");
    if (!std::isfinite(slack)) return fail(FRX_ERR_INVALID_ARG, "slack must be finite");
    if (frx_device_count() < 1) return frx::no_device();
    HIP_TRY(hipSetDevice(p->device));
    FRX_TRY(piece_rows(p));
    FRX_TRY(stage_TC(p, T, C));
    FRX_TRY(frx_trajectory_contain_device(p, p->d_T.p, p->d_C.p, slack, p->d_rows.p, p->stream));
    FRX_TRY(fetch_rows(p, p->d_rows.p, (size_t)FRX_CONTAIN_FIELDS * p->P, piece_out));
    frx::fold_contain(p->B, p->poff.data(), T, p->h_out20.p, cand_out, flags);
    return FRX_OK;
}

// ---- clearance ----
int frx_trajectory_clearance_workspace(frx_problem *p, int intervals, int n_obs, size_t *bytes) {
    if (!p || !bytes) return fail(FRX_ERR_INVALID_ARG, "null argument");
    int chunk = 0, nchunks = 0;
    FRX_TRY(clear_split(p, intervals, n_obs, &chunk, &nchunks));
    *bytes = sizeof(double) * clear_work(p, nchunks);
    return FRX_OK;
}

int frx_trajectory_clearance_device(frx_problem *p, const double *T_dev, const double *C_dev, int intervals, int n_obs, const double *obs_dev, void *work_dev,
                                    double *piece_out_dev, void *hip_stream) {
    if (!p || !T_dev || !C_dev || !obs_dev || !piece_out_dev) return fail(FRX_ERR_INVALID_ARG, "null argument");
    int chunk = 0, nchunks = 0;
    FRX_TRY(clear_split(p, intervals, n_obs, &chunk, &nchunks));
    if (nchunks > 1 && !work_dev) return fail(FRX_ERR_INVALID_ARG, "work_dev is NULL and frx_trajectory_clearance_workspace asks for scratch");
    HIP_TRY((hipError_t)frx::launch_clear(p->dp, T_dev, C_dev, intervals, n_obs, obs_dev, chunk, nchunks, (double *)work_dev, piece_out_dev, hip_stream));
    return FRX_OK;
}

int frx_trajectory_clearance(frx_problem *p, const double *T, const double *C, int intervals, int n_obs, const double *obs, double *piece_out, double *cand_out,
                             unsigned *flags) {
    if (!p || !T || !C || !obs || !cand_out) return fail(FRX_ERR_INVALID_ARG, "null argument");
    int chunk = 0, nchunks = 0;
    FRX_TRY(clear_split(p, intervals, n_obs, &chunk, &nchunks));
    HIP_TRY(hipSetDevice(p->device));
    const size_t n_rows = (size_t)FRX_CLEAR_FIELDS * p->P, n_work = clear_work(p, nchunks);
    const frx::Carve at = frx::carve_clear(n_rows, n_obs, n_work);
    FRX_TRY(grow(p->d_clear, at.total, "frx_trajectory_clearance"));
    p->clx_last_work = nullptr;                                              // (the buffer is laid out anew: the exact form's partials in it are gone)
    double *d_rows = p->d_clear.p, *d_obs = d_rows + at.second, *d_work = n_work ? d_rows + at.third : nullptr;
    FRX_TRY(stage_TC(p, T, C));
    HIP_TRY(hipMemcpyAsync(d_obs, obs, sizeof(double) * (at.third - at.second), hipMemcpyHostToDevice, p->stream));
    FRX_TRY(frx_trajectory_clearance_device(p, p->d_T.p, p->d_C.p, intervals, n_obs, d_obs, d_work, d_rows, p->stream));
    FRX_TRY(fetch_rows(p, d_rows, n_rows, piece_out));
    frx::fold_clearance(p->B, p->poff.data(), T, p->h_out20.p, nullptr, cand_out, flags);
    return FRX_OK;
}

// Tests: points > 0 makes every later clearance call on the handle split the cloud into chunks of that many points (the last one shorter), whatever the
// number of pieces; 0 returns to the library's own split.  The workspace query follows it.
int frx_debug_set_clear_chunk(frx_problem *p, int points) {
    if (!p || points < 0) return fail(FRX_ERR_INVALID_ARG, "null handle or a negative chunk");
    p->clear_chunk = points;
    return FRX_OK;
}

// ---- exact clearance ----
int frx_clearance_exact_fold(int B, const int *piece_off, const double *T, const double *rows, double *cand_out, unsigned *flags) {
    FRX_TRY(fold_args("frx_clearance_exact_fold", B, piece_off, T, rows));
    FRX_TRY(frx::offsets_args("frx_clearance_exact_fold: piece_off", B, piece_off, false));
    frx::fold_clearance_exact(B, piece_off, T, rows, cand_out, flags);
    return FRX_OK;
}

int frx_trajectory_clearance_exact_workspace(frx_problem *p, int n_obs, size_t *bytes) {
    if (!p || !bytes) return fail(FRX_ERR_INVALID_ARG, "null argument");
    int chunk = 0, nchunks = 0;
    FRX_TRY(clear_exact_split(p, n_obs, &chunk, &nchunks));
    *bytes = sizeof(double) * clear_exact_work(p, nchunks);
    return FRX_OK;
}

int frx_trajectory_clearance_exact_device(frx_problem *p, const double *T_dev, const double *C_dev, int n_obs, const double *obs_dev, void *work_dev,
                                          double *piece_out_dev, void *hip_stream) {
    if (!p || !T_dev || !C_dev || !obs_dev || !piece_out_dev) return fail(FRX_ERR_INVALID_ARG, "null argument");
    if (!work_dev) return fail(FRX_ERR_INVALID_ARG, "work_dev is NULL: frx_trajectory_clearance_exact_workspace says how much scratch the launches need");
    int chunk = 0, nchunks = 0;
    FRX_TRY(clear_exact_split(p, n_obs, &chunk, &nchunks));
    HIP_TRY((hipError_t)frx::launch_clear_exact(p->dp, T_dev, C_dev, n_obs, obs_dev, chunk, nchunks, p->clx_cull, (double *)work_dev, piece_out_dev, hip_stream));
    p->clx_last_work = (const double *)work_dev; p->clx_last_nchunks = nchunks;
    return FRX_OK;
}

int frx_trajectory_clearance_exact(frx_problem *p, const double *T, const double *C, int n_obs, const double *obs, double *piece_out, double *cand_out,
                                   unsigned *flags) {
    if (!p || !T || !C || !obs || !cand_out) return fail(FRX_ERR_INVALID_ARG, "null argument");
    int chunk = 0, nchunks = 0;
    FRX_TRY(clear_exact_split(p, n_obs, &chunk, &nchunks));
    HIP_TRY(hipSetDevice(p->device));
    const size_t n_rows = (size_t)FRX_CLEAR_EXACT_FIELDS * p->P;
    const frx::Carve at = frx::carve_clear(n_rows, n_obs, clear_exact_work(p, nchunks));   // (the handle's cloud buffer, as the dense form lays it out)
    FRX_TRY(grow(p->d_clear, at.total, "frx_trajectory_clearance_exact"));
    double *d_rows = p->d_clear.p, *d_obs = d_rows + at.second, *d_work = d_rows + at.third;
    FRX_TRY(stage_TC(p, T, C));
    HIP_TRY(hipMemcpyAsync(d_obs, obs, sizeof(double) * (at.third - at.second), hipMemcpyHostToDevice, p->stream));
    FRX_TRY(frx_trajectory_clearance_exact_device(p, p->d_T.p, p->d_C.p, n_obs, d_obs, d_work, d_rows, p->stream));
    FRX_TRY(fetch_rows(p, d_rows, n_rows, piece_out));
    frx::fold_clearance_exact(p->B, p->poff.data(), T, p->h_out20.p, cand_out, flags);
    return FRX_OK;
}

// Tests: points > 0 forces that many cloud points per chunk of every later exact clearance call and workspace query on the handle (0: the library's own split);
// cull_on == 0 makes every point a survivor that runs both tasks.  Rows depend on neither.
int frx_debug_set_clear_exact(frx_problem *p, int chunk_points, int cull_on) {
    if (!p || chunk_points < 0) return fail(FRX_ERR_INVALID_ARG, "null handle or a negative chunk");
    p->clx_chunk = chunk_points; p->clx_cull = cull_on ? 1 : 0;
    return FRX_OK;
}

// Tests: per piece, the points that survived the cull and the degree-21 tasks that ran in the last exact clearance call on the handle, summed over the chunks of
// the partials that call left in its workspace (which must still be alive).  Waits for the device.
int frx_debug_clear_exact_counts(frx_problem *p, int *survivors, int *ell_tasks) {
    if (!p || !survivors || !ell_tasks) return fail(FRX_ERR_INVALID_ARG, "null argument");
    if (!p->clx_last_work) return fail(FRX_ERR_INVALID_ARG, "frx_debug_clear_exact_counts: no exact clearance call on this handle since its cloud buffer was last laid out");
    HIP_TRY(hipSetDevice(p->device));
    HIP_TRY(hipDeviceSynchronize());
    const int nc = p->clx_last_nchunks;
    std::vector<double> part(clear_exact_work(p, nc));
    HIP_TRY(hipMemcpy(part.data(), p->clx_last_work, sizeof(double) * part.size(), hipMemcpyDeviceToHost));
    for (int k = 0; k < p->P; k++) {
        double s = 0.0, e = 0.0;
        for (int c = 0; c < nc; c++) { const double *w = part.data() + ((size_t)k * nc + c) * frx::CLEAR_EXACT_PARTIAL; s += w[6]; e += w[7]; }
        survivors[k] = (int)s; ell_tasks[k] = (int)e;
    }
    return FRX_OK;
}

// ---- map distance ----
int frx_map_distance_fold(int B, const int *piece_off, const double *T, const double *rows, double margin, double *cand_out, unsigned *flags) {
    FRX_TRY(fold_args("frx_map_distance_fold", B, piece_off, T, rows));
    if (margin != margin) return fail(FRX_ERR_INVALID_ARG, "frx_map_distance_fold: margin is not a number");
    FRX_TRY(frx::offsets_args("frx_map_distance_fold: piece_off", B, piece_off, false));
    frx::fold_map_distance(B, piece_off, T, rows, margin, cand_out, flags);
    return FRX_OK;
}

int frx_trajectory_map_distance_device(frx_problem *p, const double *T_dev, const double *C_dev, int intervals, const frx_voxel_map *map, const double *field_dev,
                                       double *piece_out_dev, void *hip_stream) {
    if (!p || !T_dev || !C_dev || !map || !field_dev || !piece_out_dev) return fail(FRX_ERR_INVALID_ARG, "null argument");
    FRX_TRY(map_distance_args(intervals, map));
    HIP_TRY((hipError_t)frx::launch_map_distance(p->P, T_dev, C_dev, intervals, map->origin, map->dim, map->res, field_dev, piece_out_dev, hip_stream));
    return FRX_OK;
}

int frx_trajectory_map_distance(frx_problem *p, const double *T, const double *C, int intervals, const frx_voxel_map *map, const double *field, double margin,
                                double *piece_out, double *cand_out, unsigned *flags) {
    if (!p || !T || !C || !map || !field || !cand_out) return fail(FRX_ERR_INVALID_ARG, "null argument");
    FRX_TRY(map_distance_args(intervals, map));
    if (margin != margin) return fail(FRX_ERR_INVALID_ARG, "frx_trajectory_map_distance: margin is not a number");
    HIP_TRY(hipSetDevice(p->device));
    const size_t n_rows = (size_t)FRX_MAPDIST_FIELDS * p->P;
    const frx::Carve at = frx::carve_mapdist(n_rows, map->dim);
    FRX_TRY(grow(p->d_mapdist, at.total, "frx_trajectory_map_distance"));
    double *d_rows = p->d_mapdist.p, *d_field = d_rows + at.second;
    FRX_TRY(stage_TC(p, T, C));
    HIP_TRY(hipMemcpyAsync(d_field, field, sizeof(double) * (at.third - at.second), hipMemcpyHostToDevice, p->stream));
    FRX_TRY(frx_trajectory_map_distance_device(p, p->d_T.p, p->d_C.p, intervals, map, d_field, d_rows, p->stream));
    FRX_TRY(fetch_rows(p, d_rows, n_rows, piece_out));
    frx::fold_map_distance(p->B, p->poff.data(), T, p->h_out20.p, margin, cand_out, flags);
    return FRX_OK;
}

// Tests: the fold of the blocking check (kind 0), extrema (1) and clearance (2) entries on piece rows the caller made up; no handle, no device.
int frx_debug_fold_rows(int kind, int B, const int *piece_off, const double *T, const double *rows, const double *limits, double *cand_out, unsigned *flags) {
    if (kind < 0 || kind > 2 || B < 1 || !piece_off || !T || !rows || !limits) return fail(FRX_ERR_INVALID_ARG, "kind must be 0, 1 or 2, B >= 1 and no input NULL");
    (kind == 0 ? frx::fold_check : kind == 1 ? frx::fold_extrema : frx::fold_clearance)(B, piece_off, T, rows, limits, cand_out, flags);
    return FRX_OK;
}

// ---- sample ----
int frx_trajectory_sample_device(frx_problem *p, const double *T_dev, const double *C_dev, int n_samples, double t0, double dt, const double *times_dev,
                                 double *out_dev, void *hip_stream) {
    if (!p || !T_dev || !C_dev || !out_dev) return fail(FRX_ERR_INVALID_ARG, "null argument");
    size_t n_out = 0;
    FRX_TRY(sample_args(p, n_samples, t0, dt, times_dev != nullptr, &n_out));
    if ((uintptr_t)out_dev % 16) return fail(FRX_ERR_INVALID_ARG, "out_dev must be 16-byte aligned");
    HIP_TRY((hipError_t)frx::launch_sample(p->dp, p->maxN, T_dev, C_dev, n_samples, t0, dt, times_dev, out_dev, hip_stream));
    return FRX_OK;
}

int frx_trajectory_sample(frx_problem *p, const double *T, const double *C, int n_samples, double t0, double dt, const double *times, double *out) {
    if (!p || !T || !C || !out) return fail(FRX_ERR_INVALID_ARG, "null argument");
    size_t n_out = 0;
    FRX_TRY(sample_args(p, n_samples, t0, dt, times != nullptr, &n_out));
    HIP_TRY(hipSetDevice(p->device));
    const frx::Carve at = frx::carve_sample(n_out, times != nullptr);
    if (at.total > SIZE_MAX / sizeof(double)) return fail(FRX_ERR_ALLOC, "frx_trajectory_sample: output too large");
    FRX_TRY(grow(p->d_sample, at.total, "frx_trajectory_sample"));
    double *d_out = p->d_sample.p, *d_times = times ? d_out + at.second : nullptr;
    FRX_TRY(stage_TC(p, T, C));
    if (times) HIP_TRY(hipMemcpyAsync(d_times, times, sizeof(double) * (at.third - at.second), hipMemcpyHostToDevice, p->stream));
    FRX_TRY(frx_trajectory_sample_device(p, p->d_T.p, p->d_C.p, n_samples, t0, dt, d_times, d_out, p->stream));
    HIP_TRY(hipMemcpyAsync(out, d_out, sizeof(double) * n_out, hipMemcpyDeviceToHost, p->stream));   // (the rows go to the caller as they are: no fold, no staging)
    HIP_TRY(hipStreamSynchronize(p->stream));
    return FRX_OK;
}

} // extern "C"
