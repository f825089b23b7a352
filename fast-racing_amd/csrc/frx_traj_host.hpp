// What the trajectory entries (frx_traj.cpp) decide on the host, in plain C++ (no HIP, no handle): the split of an obstacle cloud into chunks, the rule of an
// offsets array, the rules of the scalar arguments, and the carve-up of each scratch buffer the blocking forms grow.  The entries call these functions and so
// does the host build of tests/hostcheck (tests/test_traj_host_cpu.py).  Refusals go through frx::set_error as everywhere.
// (The functions are static: libfrx.so exports the C ABI, not these.)
#pragma once
#include <cmath>
#include <cstddef>
#include <string>

#include "frx_internal.hpp"

namespace frx {

// ---- the split of a cloud ----
// Points per chunk and chunks per piece for P pieces against n_obs points: force > 0 takes that many points per chunk, else enough chunks of whole multiples of
// `unit` points to reach target_wgs workgroups (one chunk when P alone does).  Both are constants of the kernel (frx_device.hpp), so the split - and with it the
// workspace - depends on (P, n_obs) alone.  0 when P x chunks does not fit a grid.
static inline int cloud_split(int P, int n_obs, int force, int unit, int target_wgs, int *chunk, int *nchunks) {
    long long c = force;
    if (force <= 0) {
        const long long want = P < target_wgs ? target_wgs / P : 1;
        c = ((long long)n_obs + want - 1) / want;
        c = (c + unit - 1) / unit * unit;
    }
    const long long nc = ((long long)n_obs + c - 1) / c;
    if ((long long)P * nc > 0x7fffffffLL) return 0;
    *chunk = (int)(c < n_obs ? c : n_obs); *nchunks = (int)nc;
    return 1;
}

// ---- offsets ----
// off [B + 1] starts at 0 (from_zero) or anywhere >= 0 and never falls.  `what` names the array, behind the entry's name where its messages carry one
// ("frx_contain_fold: piece_off", "gate_off").
static inline int offsets_args(const char *what, int B, const int *off, bool from_zero) {
    if (from_zero ? off[0] != 0 : off[0] < 0) return set_error(FRX_ERR_INVALID_ARG, std::string(what) + (from_zero ? "[0] must be 0" : "[0] must be >= 0"));
    for (int b = 0; b < B; b++)
        if (off[b + 1] < off[b]) return set_error(FRX_ERR_INVALID_ARG, std::string(what) + " must not fall (candidate " + std::to_string(b) + ")");
    return FRX_OK;
}

// ---- scalars ----
static inline int intervals_arg(int intervals) {
    if (intervals < 1 || intervals > FRX_CHECK_MAX_INTERVALS) return set_error(FRX_ERR_INVALID_ARG, "intervals must lie in 1.." + std::to_string(FRX_CHECK_MAX_INTERVALS));
    return FRX_OK;
}
static inline int cloud_points_arg(int n_obs) {
    if (n_obs < 1 || n_obs > FRX_CLEAR_MAX_POINTS) return set_error(FRX_ERR_INVALID_ARG, "n_obs must lie in 1.." + std::to_string(FRX_CLEAR_MAX_POINTS));
    return FRX_OK;
}
// the sampler's times: S samples at times [B][S] (have_times), t0 + s dt (dt > 0) or spread over each duration (dt == 0, which takes two samples at least)
static inline int sample_time_args(int n_samples, double t0, double dt, bool have_times) {
    if (n_samples < 1) return set_error(FRX_ERR_INVALID_ARG, "n_samples must be >= 1");
    if (!std::isfinite(t0) || !std::isfinite(dt) || dt < 0.0) return set_error(FRX_ERR_INVALID_ARG, "t0 and dt must be finite and dt >= 0");
    if (!have_times && dt == 0.0 && n_samples < 2) return set_error(FRX_ERR_INVALID_ARG, "n_samples must be >= 2 when dt == 0 (samples spread over each duration)");
    return FRX_OK;
}
// *n_out = B x S x FRX_SAMPLE_FIELDS, the doubles of the sampler's rows
static inline int sample_rows_arg(int B, int n_samples, size_t *n_out) {
    size_t n = 0;
    if (__builtin_mul_overflow((size_t)n_samples, (size_t)B, &n) || __builtin_mul_overflow(n, (size_t)FRX_SAMPLE_FIELDS, &n))
        return set_error(FRX_ERR_INVALID_ARG, "n_samples x B x FRX_SAMPLE_FIELDS overflows size_t");
    *n_out = n;
    return FRX_OK;
}

// ---- the scratch buffers of the blocking forms ----
// Where the second and third part of a buffer begin behind the piece rows at 0, and its length, all in doubles.
struct Carve { size_t second, third, total; };
// frx_trajectory_clearance[_exact]: the rows, the cloud [n_obs][3], then n_work doubles of partials
static inline Carve carve_clear(size_t n_rows, int n_obs, size_t n_work) { const size_t cloud = 3 * (size_t)n_obs; return {n_rows, n_rows + cloud, n_rows + cloud + n_work}; }
// frx_trajectory_gates: the rows [n_gates][FRX_GATE_FIELDS], the records [n_gates][9], then gate_off as B + 1 ints in whole doubles
static inline Carve carve_gates(int n_gates, int B) {
    const size_t rows = (size_t)FRX_GATE_FIELDS * n_gates, rec = 9 * (size_t)n_gates;
    return {rows, rows + rec, rows + rec + ((size_t)B + 2) / 2};
}
// frx_trajectory_sample: the n_out doubles of rows (first: 16-byte aligned), then one time per row when the caller brings times
static inline Carve carve_sample(size_t n_out, bool have_times) { const size_t times = have_times ? n_out / FRX_SAMPLE_FIELDS : 0; return {n_out, n_out + times, n_out + times}; }
// frx_trajectory_map_distance: the rows, then the field over the map's grid
static inline Carve carve_mapdist(size_t n_rows, const int *dim) { const size_t cells = (size_t)dim[0] * dim[1] * dim[2]; return {n_rows, n_rows + cells, n_rows + cells}; }

} // namespace frx
