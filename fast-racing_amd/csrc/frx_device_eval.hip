// hipcc translation unit: the one-launch evaluation (frx_eval_kernel.hpp) and its launcher.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cassert>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <mutex>

#define FRX_KERNEL_LINKAGE static          // the stage kernels of frx_kernels.hpp belong to frx_device.hip: here only their bodies are used
#include "frx_eval_kernel.hpp"

namespace frx {

static bool eval_argp() { static const bool on = [] { const char *e = std::getenv("FRX_EVAL_ARGPTR"); return !(e && e[0] == '0'); }(); return on; }   // FRX_EVAL_ARGPTR=0: the by-value form (A/B)
static bool eval_early_t() { static const bool on = [] { const char *e = std::getenv("FRX_EVAL_EARLY_T"); return !(e && e[0] == '0'); }(); return on; }   // FRX_EVAL_EARLY_T=0: the staged-durations form (A/B)
static bool eval_tail() { static const bool on = [] { const char *e = std::getenv("FRX_EVAL_TAIL"); return !(e && e[0] == '0'); }(); return on; }   // FRX_EVAL_TAIL=0: f and `done` behind a barrier and a status trip at the kernel's end (A/B; with the two switches above at their defaults only)
// FRX_EVAL_HANDOFF=0: the penalty partials piece-major, polled with 8-byte loads, the adjoint's multipliers requested behind the poll (A/B).  Read once per process, before the first handle
// exists (eval_cluster_geometry): the two forms put a granule at different addresses of one buffer, and a tag is only good for the address it was written to.
static bool eval_handoff() { static const bool on = [] { const char *e = std::getenv("FRX_EVAL_HANDOFF"); return !(e && e[0] == '0'); }(); return on && eval_argp() && eval_tail(); }
// FRX_EVAL_CHAIN=0: the form with the cycle stamps compiled in and every argument field loaded at its use - the one the diagnostics launch in any case (A/B; with the four
// switches above at their defaults only)
static bool eval_chain() { static const bool on = [] { const char *e = std::getenv("FRX_EVAL_CHAIN"); return !(e && e[0] == '0'); }(); return on && eval_handoff(); }
// FRX_EVAL_GEOM=0: the run-time instantiation also where the handle's geometry is the class EvalGeomK16 (A/B; with the five switches above at their defaults only)
static bool eval_geom_on() { static const bool on = [] { const char *e = std::getenv("FRX_EVAL_GEOM"); return !(e && e[0] == '0'); }(); return on && eval_handoff() && eval_early_t(); }
typedef eval_geom<EvalGeomK16> GeomK16;
// does a handle of this geometry launch the class instantiation (k_eval_cluster<.., EvalGeomK16>)?  Exactly the class's integers, nothing "close": any other handle takes the run-time form.
int eval_cluster_class(const LaunchGeom &g) {
    return (eval_geom_on() && g.ev_G && g.lpp == GeomK16::lpp && g.ppw == GeomK16::ppw && g.Kmax == GeomK16::kmax && g.pcr_steps == GeomK16::nsteps) ? 1 : 0;
}
// the instantiation of the hand-off form that carries the stamps: the diagnostics' launches, and every launch under FRX_EVAL_CHAIN=0
static const void *eval_fn_stamps() { return eval_early_t() ? (const void *)k_eval_cluster<true, true, true, true> : (const void *)k_eval_cluster<true, false, true, true>; }
// the instantiation the launcher takes: argument pointer (or not) x early durations (or not)
static const void *eval_fn() {
    if (eval_chain()) return eval_early_t() ? (const void *)k_eval_cluster<true, true, true, true, true> : (const void *)k_eval_cluster<true, false, true, true, true>;
    if (eval_handoff()) return eval_early_t() ? (const void *)k_eval_cluster<true, true, true, true> : (const void *)k_eval_cluster<true, false, true, true>;
    if (!eval_tail() && eval_argp() && eval_early_t()) return (const void *)k_eval_cluster<true, true, false>;
    return eval_argp() ? (eval_early_t() ? (const void *)k_eval_cluster<true, true> : (const void *)k_eval_cluster<true, false>)
                       : (eval_early_t() ? (const void *)k_eval_cluster<false, true> : (const void *)k_eval_cluster<false, false>);
}

// (see launch_set_limits, frx_device.hip: the dynamic-LDS limit of a kernel only grows, per device)
int eval_cluster_raise_limit(size_t bytes) {
    static std::mutex mu;
    static size_t held[64] = {};
    std::lock_guard<std::mutex> lock(mu);
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return (int)hipErrorInvalidDevice;
    if (bytes <= held[dev]) return 0;
    hipError_t e = hipFuncSetAttribute(eval_fn(), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e == hipSuccess && eval_chain()) e = hipFuncSetAttribute(eval_fn_stamps(), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);   // (the diagnostics' instantiation)
    if (e == hipSuccess && eval_geom_on()) {                             // (the class instantiations: production and diagnostics)
        e = hipFuncSetAttribute((const void *)k_eval_cluster<true, true, true, true, true, EvalGeomK16>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
        if (e == hipSuccess) e = hipFuncSetAttribute((const void *)k_eval_cluster<true, true, true, true, false, EvalGeomK16>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    }
    if (e == hipSuccess) held[dev] = bytes;
    return (int)e;
}
static int eval_pen_lds(const LaunchGeom &g) { return g.ppw * 19 + g.ppw * (g.Kmax + 1) * 4 + 64 * 21; }   // doubles per wave (penalty_body with a 64-lane group)
static_assert(GeomK16::pen_lds == 3 * 19 + 3 * 36 + 64 * 21, "the class's per-wave LDS is eval_pen_lds of its integers");
int eval_cluster_geometry(LaunchGeom &g) {
    g.ev_G = 0; g.lds_ev = 0;
    (void)eval_handoff();
    if (g.solver != SOLVER_KNOT_PCR || g.knot_threads != 64 || g.ppw < 1) return 0;
    const int ntasks = (g.maxN + g.ppw - 1) / g.ppw;
    const size_t lds = sizeof(double) * (size_t)eval_cluster_lds(g.maxN * 19, g.maxXb, g.maxVb, g.maxCN, g.pcr_steps, eval_pen_lds(g)).total;
    if (lds > (size_t)160 * 1024) return 0;
    g.ev_G = 1 + (ntasks + 3) / 4;                                   // the members take every wave-task of the largest candidate in one pass
    g.lds_ev = lds;
    return g.ev_G;
}
int eval_cluster_blocks_per_cu(size_t lds_bytes) {
    int n = 0;
    const void *fn = eval_fn();
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, fn, 256, lds_bytes) != hipSuccess) { (void)hipGetLastError(); return 0; }
    return n;
}
size_t eval_cluster_args_bytes() { return sizeof(EvalClusterArgs); }
// The handle's constant arguments (frx_api.cpp keeps a host copy next to a device copy, uploaded at create, and a second pair with the stamps pointer set that the
// diagnostics upload before their evaluation): everything launch_eval_cluster used to pack per call.
void eval_cluster_args(const DevProblem &dp, const LaunchGeom &g, double *T, double *C, unsigned long long *ll, unsigned *words, void *out) {
    EvalClusterArgs a;
    std::memset(&a, 0, sizeof(a));
    assert(!eval_handoff() || (reinterpret_cast<uintptr_t>(ll) & 15u) == 0);   // value-major granules travel as 16-byte stores and loads (the buffer is a device allocation of its own: 256-byte aligned)
    a.dp = dp; a.T = T; a.C = C; a.out20ll = ll; a.words = words; a.status = words + (size_t)64 * dp.B;
    a.G = g.ev_G; a.maxCN = g.maxCN; a.maxXb = g.maxXb; a.maxVb = g.maxVb; a.nsteps = g.pcr_steps; a.lpp = g.lpp; a.ppw = g.ppw; a.Kmax = g.Kmax; a.pen_lds = eval_pen_lds(g); a.maxN19 = g.maxN * 19;
    std::memcpy(out, &a, sizeof(a));
}
int launch_eval_cluster(const LaunchGeom &g, int B, const void *args_host, const void *args_dev, const double *x, double *f, double *grad,
                        unsigned long long timeout_ticks, void *stream, unsigned *status_host) {
    if (!g.ev_G) return (int)hipErrorInvalidValue;
    EvalCallArgs c;
    c.x = x; c.f = f; c.g = grad; c.status_host = status_host; c.timeout_ticks = timeout_ticks;
    { const char *e = std::getenv("FRX_EVAL_FUSED_WT"); c.force_wt = (e && e[0] == '1') ? 1 : 0; }
    c.test_drop_members = timeout_ticks == 1ull ? 1 : 0;               // (test mode, frx_debug_set_eval_fused(p, 2): members that never arrive and a 50 us bound)
    if (c.test_drop_members) c.timeout_ticks = 5000ull;
    const dim3 grid(8 * g.ev_G * ((B + 7) / 8));
    const bool et = eval_early_t();
    // the production instantiation has no stamp code: a handle whose stamps pointer is set (a diagnostic's evaluation) takes the one that has, with the argument block that carries the pointer
    if (eval_cluster_class(g) && args_dev) {                           // the geometry class: its production instantiation, or the one with the stamps under the same rule as below
        assert(((const EvalClusterArgs *)args_host)->pen_lds == GeomK16::pen_lds && ((const EvalClusterArgs *)args_host)->nsteps == GeomK16::nsteps);
        if (eval_chain() && !((const EvalClusterArgs *)args_host)->dp.stamps) hipLaunchKernelGGL((k_eval_cluster<true, true, true, true, true, EvalGeomK16>), grid, dim3(256), g.lds_ev, (hipStream_t)stream, (const EvalClusterArgs *)args_dev, c);
        else hipLaunchKernelGGL((k_eval_cluster<true, true, true, true, false, EvalGeomK16>), grid, dim3(256), g.lds_ev, (hipStream_t)stream, (const EvalClusterArgs *)args_dev, c);
    } else if (eval_chain() && args_dev && !((const EvalClusterArgs *)args_host)->dp.stamps) {
        if (et) hipLaunchKernelGGL((k_eval_cluster<true, true, true, true, true>), grid, dim3(256), g.lds_ev, (hipStream_t)stream, (const EvalClusterArgs *)args_dev, c);
        else hipLaunchKernelGGL((k_eval_cluster<true, false, true, true, true>), grid, dim3(256), g.lds_ev, (hipStream_t)stream, (const EvalClusterArgs *)args_dev, c);
    } else if (eval_handoff() && args_dev) {
        if (et) hipLaunchKernelGGL((k_eval_cluster<true, true, true, true>), grid, dim3(256), g.lds_ev, (hipStream_t)stream, (const EvalClusterArgs *)args_dev, c);
        else hipLaunchKernelGGL((k_eval_cluster<true, false, true, true>), grid, dim3(256), g.lds_ev, (hipStream_t)stream, (const EvalClusterArgs *)args_dev, c);
    } else if (eval_argp() && args_dev) {
        if (et && !eval_tail()) hipLaunchKernelGGL((k_eval_cluster<true, true, false>), grid, dim3(256), g.lds_ev, (hipStream_t)stream, (const EvalClusterArgs *)args_dev, c);
        else if (et) hipLaunchKernelGGL((k_eval_cluster<true, true>), grid, dim3(256), g.lds_ev, (hipStream_t)stream, (const EvalClusterArgs *)args_dev, c);
        else hipLaunchKernelGGL((k_eval_cluster<true, false>), grid, dim3(256), g.lds_ev, (hipStream_t)stream, (const EvalClusterArgs *)args_dev, c);
    } else {
        if (et) hipLaunchKernelGGL((k_eval_cluster<false, true>), grid, dim3(256), g.lds_ev, (hipStream_t)stream, *(const EvalClusterArgs *)args_host, c);
        else hipLaunchKernelGGL((k_eval_cluster<false, false>), grid, dim3(256), g.lds_ev, (hipStream_t)stream, *(const EvalClusterArgs *)args_host, c);
    }
    return (int)hipGetLastError();
}
} // namespace frx
