// hipcc translation unit: the gfx950 stage kernels, the L-BFGS vector kernels and their launchers.
// (The resident round kernel and the one-launch evaluation have translation units of their own - frx_device_round.hip, frx_device_eval.hip; the corridor kernels are in frx_device_chain.hip - so that the three
// compile side by side: k_round's six instantiations alone take longer than everything else together.)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <mutex>

#include "frx_kernels.hpp"
#include "frx_launch_forms.hpp"
#include "frx_lbfgs_kernels.hpp"

namespace frx {

// (frx_device.hpp) one table for every kernel of the library (LdsLimits, frx_launch_forms.hpp: grow-only per device and function), under one mutex
int raise_lds_limit(const void *fn, size_t bytes) {
    static std::mutex mu;
    static LdsLimits limits;
    if (!bytes) return 0;
    std::lock_guard<std::mutex> lock(mu);
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return (int)hipErrorInvalidDevice;
    return limits.raise(dev, fn, bytes, [](const void *f, size_t n) { return (int)hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)n); });
}
// the stage kernel of the penalty integral by its form (frx_launch_forms.hpp): f(kernel)
template <class F> static int with_penalty_kernel(PenaltyForm form, F &&f) {
    switch (form) {
    case PEN_THR: return f(k_penalty);
    case PEN_LAT: return f(k_penalty_lat);
    case PEN_LAT2_17: return f(k_penalty_lat2<17>);
    case PEN_LAT2_49: return f(k_penalty_lat2<49>);
    case PEN_LAT2_0: return f(k_penalty_lat2<0>);
    case PEN_LAT2_R5: return f(k_penalty_lat2_r5);
    }
    return (int)hipErrorInvalidValue;
}
int launch_set_limits(const LaunchGeom &g) {
    int e;
    if ((e = raise_lds_limit((const void *)k_forward, g.lds_fwd))) return e;
    if ((e = raise_lds_limit((const void *)k_backward, g.lds_bwd))) return e;
    // every penalty form launch_penalty can take for this geometry: the one-phase forms, and with lds_pen2 the two-phase instantiation of its lpp and the round-5 form
    for (PenaltyForm form : {PEN_THR, PEN_LAT, penalty_lat2_form(g.lpp), PEN_LAT2_R5}) {
        const size_t bytes = form == PEN_THR || form == PEN_LAT ? g.lds_pen : g.lds_pen2;
        if (!bytes) continue;
        if ((e = with_penalty_kernel(form, [&](auto kernel) { return raise_lds_limit((const void *)kernel, bytes); }))) return e;
    }
    if ((e = raise_lds_limit((const void *)k_forward_knot, g.lds_kfwd))) return e;
    if ((e = raise_lds_limit((const void *)k_backward_knot, g.lds_kbwd))) return e;
    if ((e = raise_lds_limit((const void *)k_forward_knot64, g.lds_kfwd))) return e;
    if ((e = raise_lds_limit((const void *)k_backward_knot64, g.lds_kbwd))) return e;
    if (g.ev_G && (e = eval_cluster_raise_limit(g.lds_ev))) return e;                   // (frx_device_eval.hip: the kernel lives in that translation unit)
    return 0;
}
int launch_forward(const DevProblem &dp, const LaunchGeom &g, const double *x, double *T, double *C, double *band, void *stream) {
    if (g.solver == SOLVER_KNOT_PCR)
        if (g.knot_threads == 64) hipLaunchKernelGGL(k_forward_knot64, dim3(dp.B), dim3(256), g.lds_kfwd, (hipStream_t)stream, dp, x, T, C, g.maxCN, g.maxXb, g.maxVb, g.pcrw, g.pcr_steps);
        else hipLaunchKernelGGL(k_forward_knot, dim3(dp.B), dim3(256), g.lds_kfwd, (hipStream_t)stream, dp, x, T, C, g.maxCN, g.maxXb, g.maxVb, g.knot_threads, g.pcrw, g.pcr_steps);
    else
        hipLaunchKernelGGL(k_forward, dim3(dp.B), dim3(64), g.lds_fwd, (hipStream_t)stream, dp, x, T, C, band, g.maxN, g.maxCN);
    return (int)hipGetLastError();
}
int launch_penalty(const DevProblem &dp, const LaunchGeom &g, const double *T, const double *C, double *out20, void *stream) {
    // default: the latency form (148 VGPRs, 3 waves per SIMD, phases interleaved by the scheduler) - measured faster at the headline batch
    // (4.97 vs 5.23 us) AND at 1024 candidates (39.8 vs 42.3 us) than the throughput form (126 VGPRs, 4 waves per SIMD); FRX_PENALTY_FORM=thr selects that one
    static const int forced = [] { const char *e = std::getenv("FRX_PENALTY_FORM"); return !e ? 0 : e[0] == 'l' ? 1 : 2; }();
    const char *tp_env = std::getenv("FRX_PENALTY_TWOPHASE");           // (read per launch: the test toggles it inside one process)
    const PenaltyForm form = penalty_form(g.lds_pen2 != 0, g.lpp, forced, tp_env ? tp_env[0] : 0);
    const bool one_phase = form == PEN_THR || form == PEN_LAT;         // (the two-phase forms: pen_w == 4, 256 threads)
    return with_penalty_kernel(form, [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3((dp.P + g.ppg - 1) / g.ppg), dim3(one_phase ? 64 * g.pen_w : 256), one_phase ? g.lds_pen : g.lds_pen2, (hipStream_t)stream, dp, T, C, out20, g.lpp, g.ppg, g.Kmax);
        return (int)hipGetLastError();
    });
}
int launch_backward(const DevProblem &dp, const LaunchGeom &g, const double *x, const double *T, const double *C,
                    const double *band, const double *out20, double *f, double *grad, void *stream, const TapLaunch &t) {
    const LineSearchTap tap{t.d, t.flags, (DvResult *)t.res, t.arrive, t.flag, t.round};
    if (g.solver == SOLVER_KNOT_PCR && g.knot_threads == 64)
        hipLaunchKernelGGL(k_backward_knot64, dim3(dp.B), dim3(256), g.lds_kbwd, (hipStream_t)stream, dp, x, T, C, out20, f,
                           grad, g.maxCN, g.maxXb, g.maxVb, g.pcrw, g.pcr_steps, tap);
    else if (g.solver == SOLVER_KNOT_PCR)
        hipLaunchKernelGGL(k_backward_knot, dim3(dp.B), dim3(256), g.lds_kbwd, (hipStream_t)stream, dp, x, T, C, out20, f,
                           grad, g.maxCN, g.maxXb, g.maxVb, g.knot_threads, g.pcrw, g.pcr_steps, tap);
    else
        hipLaunchKernelGGL(k_backward, dim3(dp.B), dim3(64), g.lds_bwd, (hipStream_t)stream, dp, x, T, C, band, out20, f, grad, g.maxN,
                           g.maxCN);
    return (int)hipGetLastError();
}


static DvBuffers to_buffers(const DvLaunch &dv) {
    DvBuffers b;
    b.xoff = dv.xoff; b.x = dv.x; b.g = dv.g; b.xp = dv.xp; b.gp = dv.gp; b.d = dv.d; b.S = dv.S; b.Y = dv.Y; b.ys = dv.ys; b.gt = dv.gt; b.dflags = dv.dflags; b.pflags = dv.pflags; b.poff = dv.poff; b.m = dv.m; b.B = dv.B; b.hs = dv.hs ? (int)dv.hs : 64 * dv.W * dv.E;
    return b;
}
int launch_lbfgs_pre(const DvLaunch &dv, const void *cmd, void *res, void *stream) {
    const DvBuffers b = to_buffers(dv);
    const DvCommand *c = (const DvCommand *)cmd; DvResult *r = (DvResult *)res;
    hipStream_t st = (hipStream_t)stream;
#define FRX_PRE(E_, W_, PF_, BLK_) case ((E_ * 16 + W_) * 64 + PF_) * 8 + BLK_: hipLaunchKernelGGL((k_lbfgs_pre<E_, W_, PF_, BLK_>), dim3(dv.B), dim3(64 * W_), 0, st, b, c, r); break;
    switch (((dv.E * 16 + dv.W) * 64 + dv.PF) * 8 + dv.BLK) {
    FRX_PRE(2, 1, 16, 4) FRX_PRE(2, 2, 16, 4) FRX_PRE(2, 3, 16, 4) FRX_PRE(2, 4, 16, 4) FRX_PRE(2, 5, 16, 4) FRX_PRE(2, 6, 16, 4) FRX_PRE(2, 7, 16, 4) FRX_PRE(2, 8, 16, 4)
    FRX_PRE(4, 1, 8, 4) FRX_PRE(4, 2, 8, 4) FRX_PRE(4, 3, 8, 4) FRX_PRE(4, 4, 8, 4) FRX_PRE(4, 5, 8, 4) FRX_PRE(4, 6, 8, 4) FRX_PRE(4, 7, 8, 4) FRX_PRE(4, 8, 8, 4)
    FRX_PRE(6, 1, 8, 4) FRX_PRE(6, 2, 8, 4) FRX_PRE(6, 3, 8, 4) FRX_PRE(6, 4, 8, 4) FRX_PRE(6, 5, 8, 4) FRX_PRE(6, 6, 8, 4) FRX_PRE(6, 7, 8, 4) FRX_PRE(6, 8, 8, 4)
    FRX_PRE(8, 1, 4, 4) FRX_PRE(8, 2, 4, 4) FRX_PRE(8, 3, 4, 4) FRX_PRE(8, 4, 4, 4) FRX_PRE(8, 5, 4, 4) FRX_PRE(8, 6, 4, 4) FRX_PRE(8, 7, 4, 4) FRX_PRE(8, 8, 4, 4)
    FRX_PRE(4, 3, 8, 1) FRX_PRE(4, 3, 8, 2) FRX_PRE(2, 6, 16, 1)     // experiments (FRX_DV_GEOM)
    default: return (int)hipErrorInvalidValue;
    }
#undef FRX_PRE
    return (int)hipGetLastError();
}
int launch_lbfgs_post(const DvLaunch &dv, const double *f, const void *cmd, void *res, void *stream) {
    hipLaunchKernelGGL(k_lbfgs_post, dim3(dv.B), dim3(64), 0, (hipStream_t)stream, to_buffers(dv), f, (const DvCommand *)cmd, (DvResult *)res);
    return (int)hipGetLastError();
}


// Diagnostic (bench): the shader clock the device SUSTAINS under a latency-bound FP64 load like the round kernel's - one lone wave per CU on every CU running a
// dependent FMA chain for ~`ms` milliseconds - as shader cycles (s_memtime) per tick of the constant 100 MHz counter.  Boxes of the pool differ by 3-6 % per round
// with the SAME code object (profiles/NOTES.md); a round is a chain of dependent instructions, so its time is cycles / clock, and this is the clock.
__global__ __launch_bounds__(64) void k_clock_probe(double *out, unsigned long long *stamps, unsigned long long ticks) {
    const unsigned long long w0 = wall_clock64(), c0 = __builtin_readcyclecounter();
    double a = 1.0 + threadIdx.x * 1e-9, b = 0.999999999;
    unsigned long long w1 = w0;
    while (w1 - w0 < ticks) {
#pragma unroll
        for (int i = 0; i < 256; i++) a = __builtin_fma(a, b, 1e-12);
        w1 = wall_clock64();
    }
    const unsigned long long c1 = __builtin_readcyclecounter();
    if (threadIdx.x == 0) { stamps[2 * blockIdx.x] = c1 - c0; stamps[2 * blockIdx.x + 1] = w1 - w0; }
    if (a == 12345.678) out[0] = a;                                      // (keeps the chain)
}
int launch_clock_probe(double *out, unsigned long long *stamps, int blocks, unsigned long long ticks, void *stream) {
    hipLaunchKernelGGL(k_clock_probe, dim3(blocks), dim3(64), 0, (hipStream_t)stream, out, stamps, ticks);
    return (int)hipGetLastError();
}

} // namespace frx
