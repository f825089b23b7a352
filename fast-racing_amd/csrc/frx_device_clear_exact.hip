// hipcc translation unit: the exact clearance certificate of a batch of trajectories against the obstacle cloud (frx_clear_exact_kernel.hpp) and its launcher.
#include <hip/hip_runtime.h>

#include "frx_clear_exact_kernel.hpp"
#include "frx_device.hpp"

namespace frx {

static_assert((int)CLX_ROW == (int)CLEAR_EXACT_FIELDS && (int)CLX_PART == (int)CLEAR_EXACT_PARTIAL, "frx_device.hpp and the kernel agree");

int launch_clear_exact(const DevProblem &dp, const double *T, const double *C, int n_obs, const double *obs, int chunk, int nchunks, int cull, double *work,
                       double *rows, void *stream) {
    if (n_obs < 1 || chunk < 1 || nchunks < 1 || (long long)chunk * nchunks < n_obs || (long long)chunk * (nchunks - 1) >= n_obs ||
        (long long)dp.P * nchunks > 0x7fffffffLL || !work)
        return (int)hipErrorInvalidValue;
    ClxArgs a;
    a.P = dp.P; a.n_obs = n_obs; a.chunk = chunk; a.nchunks = nchunks; a.cull = cull;
    a.g = dp.pc.gAcc; a.eh = dp.pc.ell[0]; a.ev = dp.pc.ell[2];
    hipLaunchKernelGGL(k_traj_clear_exact_bounds, dim3((unsigned)(dp.P * nchunks)), dim3(64), 0, (hipStream_t)stream, a, T, C, obs, work);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(k_traj_clear_exact, dim3((unsigned)(dp.P * nchunks)), dim3(64), 0, (hipStream_t)stream, a, T, C, obs, work, rows);
    e = hipGetLastError();
    if (e != hipSuccess || nchunks == 1) return (int)e;
    hipLaunchKernelGGL(k_traj_clear_exact_reduce, dim3((unsigned)dp.P), dim3(64), 0, (hipStream_t)stream, dp.P, nchunks, (const double *)work, rows);
    return (int)hipGetLastError();
}

} // namespace frx
