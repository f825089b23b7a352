// hipcc translation unit: the exact gate passage certificate of a batch of trajectories (frx_gates_kernel.hpp) and its launcher.
#include <hip/hip_runtime.h>

#include "frx_gates_kernel.hpp"
#include "frx_device.hpp"

namespace frx {

static_assert((int)GATE_ROW == (int)GATE_FIELDS, "frx_device.hpp and the kernel agree");
static_assert(sizeof(double) * GATE_SLOTS * 64 < 64 * 1024, "static LDS stays under what a kernel gets without asking");

int launch_gates(int B, const int *poff, double g_acc, const double *ell, const double *T, const double *C, int n_gates, const int *gate_off,
                 const double *gates, double *out, void *stream) {
    if (B < 1 || n_gates < 1) return (int)hipErrorInvalidValue;
    const GateEll e = {{ell[0], ell[1], ell[2]}};
    hipLaunchKernelGGL(k_traj_gates, dim3(n_gates), dim3(64), 0, (hipStream_t)stream, B, poff, g_acc, e, T, C, gate_off, gates, out);
    return (int)hipGetLastError();
}

} // namespace frx
