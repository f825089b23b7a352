// hipcc translation unit: one workgroup per candidate, one launch per evaluation (frx_solo_kernel.hpp) and its launcher.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>

#define FRX_KERNEL_LINKAGE static          // the stage kernels of frx_kernels.hpp belong to frx_device.hip: here only their bodies are used
#include "frx_solo_kernel.hpp"

namespace frx {

// the instantiation of a geometry (the two boundary resolutions kappa = 16 / 48 have their own): f(kernel)
template <class F> static int with_solo_kernel(int lpp, F &&f) { return lpp == 17 ? f(k_eval_solo<17>) : lpp == 49 ? f(k_eval_solo<49>) : f(k_eval_solo<0>); }

// fills g.lds_solo (0: this geometry keeps the stage kernels): candidates of <= 64 pieces on the knot solver, one quadrature sample per lane
int eval_solo_geometry(LaunchGeom &g, int samples_per_piece) {
    g.lds_solo = 0;
    // (one quadrature sample per lane: with kappa + 1 > 64 a lane of the stage kernel walks over several samples - k_penalty_lat's loop, not this kernel's passes)
    if (g.solver != SOLVER_KNOT_PCR || g.knot_threads != 64 || samples_per_piece > 64 || g.lpp != samples_per_piece || g.lpp < 1) return 0;
    if (g.maxXb + 16 > (int)SOLO_RB) return 0;                             // (the search direction of a round's tap is parked in the bodies' row buffer)
    const size_t lds = sizeof(double) * (size_t)solo_lds(g.maxN, g.maxXb, g.maxVb, g.maxCN, g.pcr_steps, 256 / g.lpp, g.Kmax).total;
    if (lds > (size_t)160 * 1024) return 0;
    g.lds_solo = lds;
    return 1;
}
int eval_solo_raise_limit(const LaunchGeom &g) {
    if (!g.lds_solo) return 0;
    return with_solo_kernel(g.lpp, [&](auto kernel) { return raise_lds_limit((const void *)kernel, g.lds_solo); });
}
int eval_solo_blocks_per_cu(const LaunchGeom &g) {
    int n = 0;
    if (!g.lds_solo) return 0;
    (void)with_solo_kernel(g.lpp, [&](auto kernel) {
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, (const void *)kernel, 256, g.lds_solo) != hipSuccess) { (void)hipGetLastError(); n = 0; }
        return 0;
    });
    return n;
}
int launch_eval_solo(const DevProblem &dp, const LaunchGeom &g, const double *x, double *T, double *C, double *out20, double *f, double *grad, void *stream,
                     const TapLaunch &t) {
    if (!g.lds_solo) return (int)hipErrorInvalidValue;
    SoloArgs a;
    a.x = x; a.T = T; a.C = C; a.out20 = out20; a.f = f; a.g = grad; a.pcrw = g.pcrw;
    a.maxCN = g.maxCN; a.maxXb = g.maxXb; a.maxVb = g.maxVb; a.nsteps = g.pcr_steps; a.lpp = g.lpp; a.ppg = 256 / g.lpp; a.Kmax = g.Kmax; a.maxN = g.maxN;
    const LineSearchTap tap{t.d, t.flags, (DvResult *)t.res, t.arrive, t.flag, t.round};
    return with_solo_kernel(g.lpp, [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(dp.B), dim3(256), g.lds_solo, (hipStream_t)stream, dp, a, tap);
        return (int)hipGetLastError();
    });
}
} // namespace frx
