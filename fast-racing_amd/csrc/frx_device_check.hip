// hipcc translation unit: the dense feasibility check of a batch of trajectories (frx_check_kernel.hpp) and its launcher.
#include <hip/hip_runtime.h>

#include "frx_check_kernel.hpp"

namespace frx {

static constexpr int CHECK_WAVES = 4;                  // waves per workgroup
static constexpr int CHECK_WAVE_LDS_CAP = 2048;        // doubles of LDS per wave (16 KB: a workgroup stays within the default 64 KB)

int check_geometry(int intervals, int Kmax, int *lpp, int *ppw) {
    const int S = intervals + 1, hstride = (Kmax + 1) * 4;
    int l = 2;
    while (l < S && l < 64) l <<= 1;                   // the smallest power of two that holds the samples, at most a wave
    while (l < 64 && check_wave_lds(64 / l, hstride) > CHECK_WAVE_LDS_CAP) l <<= 1;   // fewer pieces per wave when their corridor blocks are large
    if (check_wave_lds(64 / l, hstride) > CHECK_WAVE_LDS_CAP) return 0;
    *lpp = l; *ppw = 64 / l;
    return 1;
}

int launch_check(const DevProblem &dp, int Kmax, const double *T, const double *C, int intervals, double *out, void *stream) {
    int lpp = 0, ppw = 0;
    if (intervals < 1 || !check_geometry(intervals, Kmax, &lpp, &ppw)) return (int)hipErrorInvalidValue;
    const int hstride = (Kmax + 1) * 4, per_wg = CHECK_WAVES * ppw;
    const size_t lds = sizeof(double) * (size_t)CHECK_WAVES * check_wave_lds(ppw, hstride);
    hipLaunchKernelGGL(k_traj_check, dim3((dp.P + per_wg - 1) / per_wg), dim3(64 * CHECK_WAVES), lds, (hipStream_t)stream, dp, T, C, intervals, out, lpp, ppw, hstride);
    return (int)hipGetLastError();
}

} // namespace frx
