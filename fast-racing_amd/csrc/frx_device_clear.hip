// hipcc translation unit: the clearance of a batch of trajectories against the obstacle cloud (frx_clear_kernel.hpp) and its launcher.
#include <hip/hip_runtime.h>

#include "frx_clear_kernel.hpp"

namespace frx {

int launch_clear(const DevProblem &dp, const double *T, const double *C, int intervals, int n_obs, const double *obs, int chunk, int nchunks,
                 double *work, double *rows, void *stream) {
    if (intervals < 1 || n_obs < 1 || chunk < 1 || nchunks < 1 || (long long)chunk * nchunks < n_obs || (long long)chunk * (nchunks - 1) >= n_obs ||
        (long long)dp.P * nchunks > 0x7fffffffLL || (nchunks > 1 && !work))
        return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_traj_clear, dim3((unsigned)(dp.P * nchunks)), dim3(CLEAR_THREADS), 0, (hipStream_t)stream, dp, T, C, intervals, obs, n_obs, chunk, nchunks,
                       work, rows);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || nchunks == 1) return (int)e;
    const int per_wg = CLEAR_THREADS / 64;
    hipLaunchKernelGGL(k_traj_clear_reduce, dim3((dp.P + per_wg - 1) / per_wg), dim3(CLEAR_THREADS), 0, (hipStream_t)stream, dp.P, T, intervals,
                       (const double *)work, nchunks, rows);
    return (int)hipGetLastError();
}

} // namespace frx
