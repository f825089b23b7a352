// hipcc translation unit: the one-launch evaluation (frx_eval_kernel.hpp) and its launcher.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cassert>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <type_traits>

#define FRX_KERNEL_LINKAGE static          // the stage kernels of frx_kernels.hpp belong to frx_device.hip: here only their bodies are used
#include "frx_eval_kernel.hpp"
#include "frx_launch_forms.hpp"

namespace frx {

// The FRX_EVAL_* switches (A/B; what each one means with the others: EvalSwitches, frx_launch_forms.hpp), read once per process, before the first handle exists
// (eval_cluster_geometry): the two forms of the hand-off put a granule at different addresses of one buffer, and a tag is only good for the address it was written to.
//   FRX_EVAL_ARGPTR=0   the by-value form
//   FRX_EVAL_EARLY_T=0  the staged-durations form
//   FRX_EVAL_TAIL=0     f and `done` behind a barrier and a status trip at the kernel's end
//   FRX_EVAL_HANDOFF=0  the penalty partials piece-major, polled with 8-byte loads, the adjoint's multipliers requested behind the poll
//   FRX_EVAL_CHAIN=0    the form with the cycle stamps compiled in and every argument field loaded at its use - the one the diagnostics launch in any case
//   FRX_EVAL_GEOM=0     the run-time instantiation also where the handle's geometry is the class EvalGeomK16
//   FRX_EVAL_FRONT=0    the front that walks the offset tables, in every form that has the argument pointer and early durations
//   FRX_EVAL_PRELUDE=0  the forward map's prelude as it was (the axis waves' staging loads and stores each behind a test of its own), in every form that has the two-trip
//                       front and the value-major hand-off
//   FRX_EVAL_ADJOINT=0  the leader's adjoint as it was (its top through the offset tables, the waypoint layer's operands requested behind the solve), in every form that
//                       has the shortened prelude on
static const EvalSwitches &eval_switches() {
    static const EvalSwitches s{!env_off("FRX_EVAL_ARGPTR"), !env_off("FRX_EVAL_EARLY_T"), !env_off("FRX_EVAL_TAIL"), !env_off("FRX_EVAL_HANDOFF"), !env_off("FRX_EVAL_CHAIN"), !env_off("FRX_EVAL_GEOM"),
                                env_off("FRX_EVAL_FRONT"), env_off("FRX_EVAL_PRELUDE"), env_off("FRX_EVAL_ADJOINT")};
    return s;
}
typedef eval_geom<EvalGeomK16> GeomK16;
static_assert(GeomK16::pen_lds == pen_wave_doubles(GeomK16::ppw, GeomK16::kmax), "the class's per-wave LDS is pen_wave_doubles of its integers");
// is a handle of this geometry of the class (k_eval_cluster<.., EvalGeomK16>)?  Exactly the class's integers, nothing "close": any other handle takes the run-time form.
static bool eval_geom_class(const LaunchGeom &g) { return g.ev_G && g.lpp == GeomK16::lpp && g.ppw == GeomK16::ppw && g.Kmax == GeomK16::kmax && g.pcr_steps == GeomK16::nsteps; }
int eval_cluster_class(const LaunchGeom &g) { return (eval_switches().geom_on() && eval_geom_class(g)) ? 1 : 0; }
int eval_cluster_front(const LaunchGeom &g) {
    EvalClusterForm m;
    if (!g.ev_G || !eval_cluster_form(eval_switches(), eval_geom_class(g), false, true, m)) return 0;
    return (m.argp && m.et && !m.old_front) ? 1 : 0;
}
int eval_cluster_prelude(const LaunchGeom &g) {
    EvalClusterForm m;
    if (!g.ev_G || !eval_cluster_form(eval_switches(), eval_geom_class(g), false, true, m)) return 0;
    return (eval_form_has_prelude(m) && !m.old_prelude) ? 1 : 0;
}

// The instantiation of a form (frx_launch_forms.hpp): f(kernel).  THE list of the instantiations that exist: a new form of the kernel is one more line here and
// its rung in eval_cluster_form.
template <bool ARGP, bool ET, bool TAIL = true, bool HO = false, bool CH = false, class GEO = void, bool FR = false, bool PRE = false, bool ADJ = false> struct eval_inst {
    static constexpr EvalClusterForm form() { return {ARGP, ET, TAIL, HO, CH, !std::is_void<GEO>::value, ARGP && ET && !FR, ARGP && ET && FR && HO && !PRE, ARGP && ET && FR && HO && PRE && !ADJ}; }
};
template <class F> static int with_eval_kernel(const EvalClusterForm &m, F &&f) {
#define FRX_EVAL_FORM(...) if (m == eval_inst<__VA_ARGS__>::form()) return f(k_eval_cluster<__VA_ARGS__>);
    FRX_EVAL_FORM(true, true, true, true)                            // the hand-off form that carries the stamps: the diagnostics' launches, and every launch under FRX_EVAL_CHAIN=0
    FRX_EVAL_FORM(true, false, true, true)
    FRX_EVAL_FORM(true, true, true, true, true)                      // the production chain
    FRX_EVAL_FORM(true, false, true, true, true)
    FRX_EVAL_FORM(true, true, false)
    FRX_EVAL_FORM(true, true)
    FRX_EVAL_FORM(true, false)
    FRX_EVAL_FORM(false, true)                                       // by value
    FRX_EVAL_FORM(false, false)
    FRX_EVAL_FORM(true, true, true, true, true, EvalGeomK16)         // the geometry class: production and diagnostics
    FRX_EVAL_FORM(true, true, true, true, false, EvalGeomK16)
    FRX_EVAL_FORM(true, true, true, true, true, EvalGeomK16, true)   // the two-trip front (FR): every form with the argument pointer and early durations has one
    FRX_EVAL_FORM(true, true, true, true, false, EvalGeomK16, true)
    FRX_EVAL_FORM(true, true, true, true, true, void, true)
    FRX_EVAL_FORM(true, true, true, true, false, void, true)
    FRX_EVAL_FORM(true, true, false, false, false, void, true)
    FRX_EVAL_FORM(true, true, true, false, false, void, true)
    FRX_EVAL_FORM(true, true, true, true, true, EvalGeomK16, true, true)   // the shortened prelude (PRE): every form with the two-trip front and the value-major hand-off has one
    FRX_EVAL_FORM(true, true, true, true, false, EvalGeomK16, true, true)
    FRX_EVAL_FORM(true, true, true, true, true, void, true, true)
    FRX_EVAL_FORM(true, true, true, true, false, void, true, true)
    FRX_EVAL_FORM(true, true, true, true, true, EvalGeomK16, true, true, true)   // the adjoint's operands in front of the poll (ADJ): every form with the shortened prelude has one
    FRX_EVAL_FORM(true, true, true, true, false, EvalGeomK16, true, true, true)
    FRX_EVAL_FORM(true, true, true, true, true, void, true, true, true)
    FRX_EVAL_FORM(true, true, true, true, false, void, true, true, true)
#undef FRX_EVAL_FORM
    return (int)hipErrorInvalidValue;                                 // (a form nobody instantiated)
}
// the form of an evaluation without the stamps on a handle outside the class: the one the occupancy query asks about
static EvalClusterForm eval_plain_form() { EvalClusterForm m; (void)eval_cluster_form(eval_switches(), false, false, true, m); return m; }

int eval_cluster_adjoint(const LaunchGeom &g) {
    EvalClusterForm m;
    if (!g.ev_G || !eval_cluster_form(eval_switches(), eval_geom_class(g), false, true, m)) return 0;
    return (eval_form_has_adjoint(m) && !m.old_adjoint) ? 1 : 0;
}
int eval_cluster_raise_limit(size_t bytes) {
    EvalClusterForm forms[4];
    const int n = eval_cluster_raised_forms(eval_switches(), forms);
    for (int i = 0; i < n; i++)
        if (const int e = with_eval_kernel(forms[i], [&](auto kernel) { return raise_lds_limit((const void *)kernel, bytes); })) return e;
    return 0;
}
int eval_cluster_geometry(LaunchGeom &g) {
    g.ev_G = 0; g.lds_ev = 0;
    (void)eval_switches();
    if (g.solver != SOLVER_KNOT_PCR || g.knot_threads != 64 || g.ppw < 1) return 0;
    const int ntasks = (g.maxN + g.ppw - 1) / g.ppw;
    const size_t lds = sizeof(double) * (size_t)eval_cluster_lds(g.maxN * 19, g.maxXb, g.maxVb, g.maxCN, g.pcr_steps, pen_wave_doubles(g.ppw, g.Kmax)).total;
    if (lds > (size_t)160 * 1024) return 0;
    g.ev_G = 1 + (ntasks + 3) / 4;                                   // the members take every wave-task of the largest candidate in one pass
    g.lds_ev = lds;
    return g.ev_G;
}
int eval_cluster_blocks_per_cu(size_t lds_bytes) {
    int n = 0;
    (void)with_eval_kernel(eval_plain_form(), [&](auto kernel) {
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, (const void *)kernel, 256, lds_bytes) != hipSuccess) { (void)hipGetLastError(); n = 0; }
        return 0;
    });
    return n;
}
size_t eval_cluster_args_bytes() { return sizeof(EvalClusterArgs); }
// The handle's constant arguments (frx_api.cpp keeps a host copy next to a device copy, uploaded at create, and a second pair with the stamps pointer set that the
// diagnostics upload before their evaluation): everything launch_eval_cluster used to pack per call.
void eval_cluster_args(const DevProblem &dp, const LaunchGeom &g, double *T, double *C, unsigned long long *ll, unsigned *words, const void *front_dev, void *out) {
    EvalClusterArgs a;
    std::memset(&a, 0, sizeof(a));
    assert(!eval_switches().handoff_on() || (reinterpret_cast<uintptr_t>(ll) & 15u) == 0);   // value-major granules travel as 16-byte stores and loads (the buffer is a device allocation of its own: 256-byte aligned)
    a.dp = dp; a.T = T; a.C = C; a.out20ll = ll; a.words = words; a.status = words + (size_t)64 * dp.B;
    a.G = g.ev_G; a.maxCN = g.maxCN; a.maxXb = g.maxXb; a.maxVb = g.maxVb; a.nsteps = g.pcr_steps; a.lpp = g.lpp; a.ppw = g.ppw; a.Kmax = g.Kmax; a.pen_lds = pen_wave_doubles(g.ppw, g.Kmax); a.maxN19 = g.maxN * 19;
    a.front = (const EvalFront *)front_dev;
    EvalArgsLead &l = a.lead;                                         // the leading lines: copies (EvalArgsLead, frx_eval_kernel.hpp)
    l.piece_coarse = dp.piece_coarse; l.piece_iv = dp.piece_iv; l.wp_nv = dp.wp_nv; l.wp_vbeg = dp.wp_vbeg; l.wp_xbeg = dp.wp_xbeg;
    l.vrec = dp.vrec; l.hblk = dp.hblk; l.headPVA = dp.headPVA; l.tailPVA = dp.tailPVA; l.status = a.status; l.words = a.words;
    l.maxN19 = a.maxN19; l.maxXb = a.maxXb; l.maxVb = a.maxVb; l.maxCN = a.maxCN; l.nsteps = a.nsteps; l.pen_lds = a.pen_lds; l.ppw = a.ppw; l.Kmax = a.Kmax; l.soft = dp.soft; l.c2 = dp.c2;
    for (int q = 0; q < 4; q++) l.chi[q] = dp.pc.chi[q];
    l.inv_kappa = dp.inv_kappa; l.out20ll = a.out20ll; l.kappa = dp.kappa;
    std::memcpy(out, &a, sizeof(a));
}
int launch_eval_cluster(const LaunchGeom &g, int B, const void *args_host, const void *args_dev, const double *x, double *f, double *grad,
                        unsigned long long timeout_ticks, void *stream, unsigned *status_host) {
    if (!g.ev_G) return (int)hipErrorInvalidValue;
    EvalCallArgs c;
    c.x = x; c.f = f; c.g = grad; c.status_host = status_host; c.timeout_ticks = timeout_ticks;
    c.force_wt = env_is("FRX_EVAL_FUSED_WT", '1') ? 1 : 0;
    c.G = (unsigned short)g.ev_G; c.B = (unsigned short)B;
    c.test_drop_members = timeout_ticks == 1ull ? 1 : 0;               // (test mode, frx_debug_set_eval_fused(p, 2): members that never arrive and a 50 us bound)
    if (c.test_drop_members) c.timeout_ticks = 5000ull;
    const dim3 grid(8 * g.ev_G * ((B + 7) / 8));
    // the production instantiation has no stamp code: a handle whose stamps pointer is set (a diagnostic's evaluation) takes the one that has, with the argument block that carries the pointer
    const EvalClusterArgs *host = (const EvalClusterArgs *)args_host;
    EvalClusterForm m;
    if (!eval_cluster_form(eval_switches(), eval_geom_class(g), host->dp.stamps != nullptr, args_dev != nullptr, m)) return (int)hipErrorInvalidValue;
    assert(!m.geo || (host->pen_lds == GeomK16::pen_lds && host->nsteps == GeomK16::nsteps));
    if (m.argp && m.et && !m.old_front) {                             // the two-trip front: the records' pointer and (G, B) in 16 bits each
        if (!host->front || g.ev_G > 0xFFFF || B > 0xFFFF) return (int)hipErrorInvalidValue;
    }
    return with_eval_kernel(m, [&](auto kernel) {
        if constexpr (std::is_same<decltype(kernel), void (*)(EvalClusterArgs, EvalCallArgs, const EvalFront *)>::value) hipLaunchKernelGGL(kernel, grid, dim3(256), g.lds_ev, (hipStream_t)stream, *host, c, host->front);
        else hipLaunchKernelGGL(kernel, grid, dim3(256), g.lds_ev, (hipStream_t)stream, (const EvalClusterArgs *)args_dev, c, host->front);
        return (int)hipGetLastError();
    });
}

// Tests (frx_debug_lane_exchange): lane_exchange<S> of frx_wave.hpp on one wave, as compiled into this translation unit - in[64] -> below[64], above[64], 64-bit
// patterns moved as they are (the kernel sees doubles, the test compares bits).
template <int S> __global__ __launch_bounds__(64) void k_lane_exchange_probe(const double *__restrict__ in, double *__restrict__ below, double *__restrict__ above) {
    const int lane = threadIdx.x;
    double lo, hi;
    lane_exchange<S>(in[lane], lo, hi);
    below[lane] = lo; above[lane] = hi;
}
int launch_lane_exchange_probe(int stride, const double *in, double *below, double *above, void *stream) {
    switch (stride) {
#define FRX_LX_PROBE(S) case S: hipLaunchKernelGGL(k_lane_exchange_probe<S>, dim3(1), dim3(64), 0, (hipStream_t)stream, in, below, above); break;
    FRX_LX_PROBE(1) FRX_LX_PROBE(2) FRX_LX_PROBE(4) FRX_LX_PROBE(8) FRX_LX_PROBE(16) FRX_LX_PROBE(32)
#undef FRX_LX_PROBE
    default: return (int)hipErrorInvalidValue;
    }
    return (int)hipGetLastError();
}
} // namespace frx
