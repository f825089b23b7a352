// hipcc translation unit: the exact corridor containment certificate of a batch of trajectories (frx_contain_kernel.hpp) and its launcher.
#include <hip/hip_runtime.h>

#include "frx_contain_kernel.hpp"
#include "frx_device.hpp"

namespace frx {

static_assert((int)CON_ROW == (int)CONTAIN_FIELDS, "frx_device.hpp and the kernel agree");
static_assert(sizeof(double) * CON_SLOTS * 64 == 33792 && sizeof(double) * CON_SLOTS * 64 < 64 * 1024, "static LDS stays under what a kernel gets without asking");

int contain_group_log2(int Kmax) {
    int lg = 0;
    while (lg < 6 && (1 << lg) < Kmax) lg++;
    return lg;
}

int launch_contain(const DevProblem &dp, int Kmax, double slack, const double *T, const double *C, double *out, void *stream) {
    if (dp.P < 1 || dp.B < 1 || Kmax < 1) return (int)hipErrorInvalidValue;
    ConArgs a;
    a.P = dp.P; a.B = dp.B; a.Kmax = Kmax; a.lg = contain_group_log2(Kmax);
    a.g = dp.pc.gAcc; a.eh = dp.pc.ell[0]; a.ev = dp.pc.ell[2]; a.margin = dp.pc.safeMargin; a.slack = slack;
    a.poff = dp.poff; a.hblk = dp.hblk;
    const int ppw = 64 >> a.lg;
    hipLaunchKernelGGL(k_traj_contain, dim3((dp.P + ppw - 1) / ppw), dim3(64), 0, (hipStream_t)stream, a, T, C, out);
    return (int)hipGetLastError();
}

} // namespace frx
