// hipcc translation unit: the exact per-piece extrema of a batch of trajectories (frx_extrema_kernel.hpp) and its launcher.
#include <hip/hip_runtime.h>

#include "frx_extrema_kernel.hpp"
#include "frx_device.hpp"

namespace frx {

static_assert((int)EXT_FIELDS == (int)EXTREMA_FIELDS, "frx_device.hpp and the kernel agree");
static_assert(sizeof(double) * EXT_SLOTS * 64 < 64 * 1024, "static LDS stays under what a kernel gets without asking");

int launch_extrema(int P, double g_acc, const double *T, const double *C, double *out, void *stream) {
    if (P < 1) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_traj_extrema, dim3((P + 63) / 64, EXT_TASKS), dim3(64), 0, (hipStream_t)stream, P, g_acc, T, C, out);
    return (int)hipGetLastError();
}

} // namespace frx
