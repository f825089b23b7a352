// C ABI (include/frx.h) of the MI355X back-end: problem set-up, batched device evaluation, the penalty on its own and the
// self-tests; the plan drivers behind frx_optimize live in frx_optimize.cpp, the trajectory entries in frx_traj.cpp.  Host-only
// translation unit (g++); the kernels live in frx_device.hip.  No CPU fallback: without a HIP device create() fails.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <thread>
#include <vector>

#include "../../include/frx.h"
#include "../../include/frx_debug.h"
#include "frx_handle.hpp"
#include "frx_launch_forms.hpp"
#include "frx_problem_tables.hpp"
#include "frx_host_pool.hpp"
#include "frx_compact.hpp"

using frx::NumaScope;

namespace {
thread_local std::string g_err = "";
}

namespace frx {

int set_error(int code, const std::string &msg) { g_err = msg; return code; }

int launch_eval(frx_problem *p, const double *x_dev, double *f_dev, double *g_dev, void *st, bool backward) {
    // a plain evaluation of a batch the chip holds at once: ONE launch (clusters of workgroups, frx_eval_kernel.hpp); the optimiser's rounds (line-search tap,
    // skipped candidates) and the diagnostics that look at stage buffers keep the three stage kernels
    //  A wait inside an earlier one-launch evaluation expired: its leader left the code in mapped host memory, and from the first launch that sees it the
    // handle takes the stage kernels by itself - also on the capturable _device form and inside the host-vector L-BFGS, which have no status check of their own.
    // No HIP call here (the caller may be capturing): the device's sticky word is cleared at the next host-synchronous point (eval_cluster_status).
    if (p->eval_fused && p->h_ev_status.p && *(volatile unsigned *)p->h_ev_status.p != 0u) { p->eval_fused_code = *(volatile unsigned *)p->h_ev_status.p; p->eval_fused = 0; }
    switch (frx::eval_route(backward, p->tap.d != nullptr, p->dp.cand_active != nullptr, p->dp.stamps != nullptr, p->eval_fused != 0, p->eval_fused_stamps != 0, p->eval_solo, p->B,
                            p->eval_solo_min_B, p->eval_solo_max_B, p->geo.lds_solo != 0, p->geo.solver == frx::SOLVER_KNOT_PCR)) {
    case frx::EVAL_CLUSTER: {
        // the handle's constant arguments live in device memory, in TWO copies: the one uploaded at create (no stamps pointer) and the one a diagnostic uploads
        // before it switches the cycle stamps on.  A launch picks the copy with the kernel's instantiation (launch_eval_cluster) and never copies anything itself:
        // the caller may be capturing, and a graph captured before a diagnostic still points at arguments nobody has touched since.
        const bool stamped = p->dp.stamps != nullptr;
        if (stamped && !p->d_ev_args_st.p) return (int)hipErrorInvalidValue;
        return frx::launch_eval_cluster(p->geo, p->B, stamped ? p->ev_args_st.data() : p->ev_args.data(), stamped ? p->d_ev_args_st.p : p->d_ev_args.p, x_dev, f_dev, g_dev, p->eval_fused_ticks, st, p->h_ev_status.p);
    }
    // batches beyond the clusters' reach (or the form forced, for tests and measurements): one workgroup per candidate runs the three stage bodies back to back - plain
    // evaluations AND the optimiser's rounds (same stage buffers, tap and skipped candidates as the three launches; bit-identical results)
    case frx::EVAL_SOLO: return frx::launch_eval_solo(p->dp, p->geo, x_dev, p->d_T.p, p->d_C.p, p->d_out20.p, f_dev, g_dev, st, p->tap);
    case frx::EVAL_STAGES: break;
    }
    int e = frx::launch_forward(p->dp, p->geo, x_dev, p->d_T.p, p->d_C.p, backward ? p->d_band.p : (double *)nullptr, st);
    if (e || !backward) return e;
    if ((e = frx::launch_penalty(p->dp, p->geo, p->d_T.p, p->d_C.p, p->d_out20.p, st))) return e;
    return frx::launch_backward(p->dp, p->geo, x_dev, p->d_T.p, p->d_C.p, p->d_band.p, p->d_out20.p, f_dev, g_dev, st, p->tap);
}

// The one-launch evaluation's sticky error word (a wait inside the launch expired: the f of the candidates concerned are NaN, so the word is only fetched when
// an objective value is not a number).  Read, cleared, reported; the handle then goes on with the stage kernels.  The stream has been synchronised by the caller.
// f == nullptr (frx_eval_status: the caller of the capturable form asks): the word is fetched whatever the objective values say.
int eval_cluster_status(frx_problem *p, const double *f) {
    if (!p->eval_fused_G || !p->d_ev_words) return FRX_OK;
    const unsigned seen = p->h_ev_status.p ? *(volatile unsigned *)p->h_ev_status.p : 0u;
    if (!p->eval_fused && !p->eval_fused_code && !seen) return FRX_OK;                  // switched off by the caller, never failed
    bool any_nan = f == nullptr || seen != 0u || p->eval_fused_code != 0u;
    for (int b = 0; f && b < p->B; b++) any_nan = any_nan || f[b] != f[b];
    if (!any_nan) return FRX_OK;
    unsigned st = 0;
    unsigned *w = p->d_ev_words + (size_t)64 * p->B;
    HIP_TRY(hipMemcpy(&st, w, sizeof(unsigned), hipMemcpyDeviceToHost));
    if (st == 0 && seen == 0u && p->eval_fused_code == 0u) return FRX_OK;
    if (st == 0) st = seen ? seen : p->eval_fused_code;
    HIP_TRY(hipMemset(w, 0, sizeof(unsigned)));
    if (p->h_ev_status.p) *(volatile unsigned *)p->h_ev_status.p = 0u;
    p->eval_fused = 0; p->eval_fused_code = 0;
    return fail(FRX_ERR_TIMEOUT, "one-launch evaluation: a wait between the workgroups of a cluster expired (code " + std::to_string(st) + "); this handle continues with one launch per stage");
}

} // namespace frx

using frx::launch_eval;
using frx::eval_cluster_status;

// ---- the steps of frx_problem_create, in the order it takes them ----
namespace {

// The handle while create builds it: every early return destroys its stream and deletes it (a finished handle leaves through frx_problem_destroy, which
// synchronises the stream first).
struct HandleOwner {
    frx_problem *p;
    explicit HandleOwner(frx_problem *q) : p(q) {}
    HandleOwner(const HandleOwner &) = delete;
    HandleOwner &operator=(const HandleOwner &) = delete;
    ~HandleOwner() {
        if (!p) return;
        if (p->stream) (void)hipStreamDestroy(p->stream);
        delete p;
    }
    frx_problem *release() { frx_problem *q = p; p = nullptr; return q; }
};

// the one place create reads the environment
frx::CreateSwitches create_switches_from_env() {
    frx::CreateSwitches s;
    if (const char *e = std::getenv("FRX_PENALTY_WAVES")) s.penalty_waves = std::atoi(e);
    if (const char *e = std::getenv("FRX_EVAL_FUSED")) s.eval_fused = e[0];
    if (const char *e = std::getenv("FRX_LOCAL_RANKS")) s.local_ranks = std::max(1, std::atoi(e));
    else if (const char *e2 = std::getenv("LOCAL_WORLD_SIZE")) s.local_ranks = std::max(1, std::atoi(e2));
    if (const char *e = std::getenv("FRX_EVAL_SOLO")) s.eval_solo = e[0];
    if (const char *e = std::getenv("FRX_EVAL_SOLO_MIN_B")) s.solo_min_B = std::atoi(e);
    if (const char *e = std::getenv("FRX_EVAL_SOLO_MAX_B")) s.solo_max_B = std::atoi(e);
    if (const char *e = std::getenv("FRX_EVAL_TIMEOUT_MS")) s.eval_timeout_ms = std::atof(e);
    s.setup_timing = std::getenv("FRX_SETUP_TIMING") != nullptr;
    return s;
}

int create_hip_error(hipError_t e, const char *step) {
    return fail(e == hipErrorOutOfMemory ? FRX_ERR_ALLOC : FRX_ERR_HIP, std::string(step) + ": " + hipGetErrorString(e));
}

// the host description of every candidate and the descriptor tables (frx_problem_tables.hpp)
int create_tables(frx_problem *p, const int *coarse_n, const double *ini_state, const double *fin_state, const int *h_off, const double *h_rec, const int *v_off,
                  const double *v_rec, frx::ProblemTables &tb) {
    frx::TablesRefusal why;
    const int rc = frx::problem_tables_fill(p->cfg, p->softT, p->B, coarse_n, ini_state, fin_state, h_off, h_rec, v_off, v_rec, p->cand, tb, &why);
    switch (why) {
    case frx::TABLES_COARSE_N: return fail(rc, "coarse_n[b] < 1");
    case frx::TABLES_NO_VERTICES: return fail(rc, "a corridor polytope has no vertices");
    case frx::TABLES_NO_HALFSPACES: return fail(rc, "an H-polytope has no half-spaces");
    case frx::TABLES_OK: break;
    }
    return FRX_OK;
}

// launch geometry + LDS budgets, the forms of the evaluation this handle takes, and the refusals of what does not fit
int create_geometry(frx_problem *p, const frx::ProblemTables &tb, const frx::CreateSwitches &sw, int ndev) {
    int cus = 256;
    { hipDeviceProp_t prop; if (hipGetDeviceProperties(&prop, p->device) == hipSuccess) cus = prop.multiProcessorCount; }
    frx::LaunchGeom &ge = p->geo;
    frx::launch_geometry_fill(ge, tb, p->cfg.qd_intervals, 4 * cus, sw.penalty_waves);
    if (!frx::eval_cluster_admitted(frx::eval_cluster_geometry(ge), p->B, cus, sw.eval_fused, sw.local_ranks, ndev)) { ge.ev_G = 0; ge.lds_ev = 0; }
    p->eval_fused_G = ge.ev_G; p->eval_fused = ge.ev_G ? 1 : 0;
    if (sw.eval_timeout_ms > 0.0) p->eval_fused_ticks = (unsigned long long)(sw.eval_timeout_ms * 1e5);
    frx::eval_solo_geometry(ge, p->cfg.qd_intervals + 1);
    const frx::SoloChoice solo = frx::eval_solo_choice(ge.lds_solo != 0, sw.eval_solo, sw.solo_min_B, sw.solo_max_B);
    p->eval_solo = solo.eval_solo; p->eval_solo_min_B = solo.min_B; p->eval_solo_max_B = solo.max_B;
    const frx::GeomVerdict v = frx::geometry_verdict(ge.knot_threads, ge.lds_kbwd, ge.lds_fwd, ge.lds_bwd, ge.lds_pen);
    if (v.refusal == frx::GEOM_KNOT_CAPACITY)
        return fail(FRX_ERR_CAPACITY, "a candidate's knot system does not fit one workgroup: " + std::to_string(ge.lds_kbwd / 1024) + " KB of LDS needed, 160 KB available (" +
                                          std::to_string(ge.knot_threads) + " knot threads, limit 256; about 128 pieces per candidate fit; the reference caps at 100, cuda_computer.cuh:24)");
    if (v.refusal == frx::GEOM_PENALTY_CAPACITY)
        return fail(FRX_ERR_CAPACITY, "piece count / half-space count too large for the LDS-resident kernels (160 KiB per CU)");
    p->banded_ok = v.banded_ok;
    if (!p->banded_ok) { ge.lds_fwd = ge.lds_bwd = 1024; }          // "unavailable" (frx_problem_set_solver), no limit to raise
    return FRX_OK;
}

hipError_t create_stream_and_limits(frx_problem *p) {
    hipError_t e;
    if ((e = hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking)) || (e = (hipError_t)frx::launch_set_limits(p->geo)) || (e = (hipError_t)frx::eval_solo_raise_limit(p->geo))) return e;
    if (p->geo.lds_solo && frx::eval_solo_blocks_per_cu(p->geo) < 1) { p->geo.lds_solo = 0; p->eval_solo = 0; }
    if (p->geo.ev_G && frx::eval_cluster_blocks_per_cu(p->geo.lds_ev) < 1) { p->geo.ev_G = 0; p->geo.lds_ev = 0; p->eval_fused_G = 0; p->eval_fused = 0; }   // (the runtime's own occupancy answer: a CU must hold a workgroup of the cluster kernel)
    return hipSuccess;
}

hipError_t upload_tables(frx_problem *p, const frx::ProblemTables &tb) {
    hipError_t e;
    if ((e = p->d_cvoff.upload(tb.cvoff)) || (e = p->d_poff.upload(tb.poff)) || (e = p->d_coff.upload(tb.coff)) || (e = p->d_xoff.upload(tb.xoff)) || (e = p->d_boff.upload(tb.boff)) ||
        (e = p->d_piece_hbeg.upload(tb.piece_hbeg)) || (e = p->d_piece_K.upload(tb.piece_K)) || (e = p->d_piece_coarse.upload(tb.piece_coarse)) || (e = p->d_piece_iv.upload(tb.piece_iv)) ||
        (e = p->d_coarse_iv.upload(tb.coarse_iv)) || (e = p->d_coarse_fbeg.upload(tb.coarse_fbeg)) ||
        (e = p->d_wp_vbeg.upload(tb.wp_vbeg)) || (e = p->d_wp_nv.upload(tb.wp_nv)) || (e = p->d_wp_xbeg.upload(tb.wp_xbeg)) ||
        (e = p->d_head.upload(tb.head)) || (e = p->d_tail.upload(tb.tail)) || (e = p->d_hblk.upload(tb.hblk)) || (e = p->d_vrec.upload(tb.vrec))) return e;
    return hipSuccess;
}

hipError_t allocate_work_space(frx_problem *p, const frx::ProblemTables &tb) {
    const size_t P = tb.P;
    hipError_t e;
    if ((e = p->d_x.alloc(tb.NX)) || (e = p->d_f.alloc(p->B)) || (e = p->d_g.alloc(tb.NX)) ||
        (e = p->d_T.alloc(P)) || (e = p->d_C.alloc(P * 18)) || (e = p->d_band.alloc(tb.boff[p->B])) || (e = p->d_out20.alloc(P * 20)) ||
        (e = p->d_pcrw.alloc((size_t)(p->geo.pcr_steps * 8 + 4) * P)) ||
        (e = p->d_wq.alloc(4 * P)) || (e = hipMemset(p->d_wq.p, 0, sizeof(double) * 4 * P))) return e;
    p->geo.pcrw = p->d_pcrw.p;
    return hipSuccess;
}

// granules, control words, the mapped status word, the argument block and the front records of the one-launch evaluation, when the handle takes it
hipError_t allocate_eval_cluster(frx_problem *p, const frx::ProblemTables &tb) {
    if (!p->eval_fused_G) return hipSuccess;
    const size_t n_ll = (size_t)40 * tb.P, n_w64 = ((size_t)64 * p->B + 2) / 2;
    hipError_t e;
    if ((e = p->d_ev_ll.alloc(n_ll + n_w64)) || (e = hipMemset(p->d_ev_ll.p, 0, sizeof(unsigned long long) * (n_ll + n_w64)))) return e;   // (not on the handle's stream: the first evaluation may come on the caller's)
    p->d_ev_words = (unsigned *)(p->d_ev_ll.p + n_ll);
    { NumaScope numa_alloc(p->device); if ((e = p->h_ev_status.alloc(16))) return e; }
    p->ev_args.assign(frx::eval_cluster_args_bytes(), 0);
    if ((e = p->d_ev_args.alloc(p->ev_args.size()))) return e;
    std::vector<frx::EvalFront> front((size_t)p->B);
    frx::eval_front_fill(p->B, tb.poff.data(), tb.coff.data(), tb.xoff.data(), tb.cvoff.data(), p->softT, p->geo.ppw, front.data());
    return p->d_ev_front.upload(front);
}

// pinned staging buffers: pages from the device's NUMA node (NumaScope)
hipError_t allocate_staging(frx_problem *p, const frx::ProblemTables &tb) {
    NumaScope numa_alloc(p->device);
    const size_t P = tb.P;
    hipError_t e;
    if ((e = p->h_x.alloc(tb.NX)) || (e = p->h_f.alloc(p->B)) || (e = p->h_g.alloc(tb.NX)) || (e = p->h_T.alloc(P)) || (e = p->h_C.alloc(P * 18)) || (e = p->h_out20.alloc(P * 20))) return e;
    return hipSuccess;
}

// what the handle keeps of the tables on the host
void adopt_tables(frx_problem *p, frx::ProblemTables &tb) {
    p->poff = std::move(tb.poff); p->coff = std::move(tb.coff); p->xoff = std::move(tb.xoff); p->boff = std::move(tb.boff); p->dimT = std::move(tb.dimT);
    p->P = tb.P; p->Pc = tb.Pc; p->NX = tb.NX; p->Kmax = tb.Kmax; p->maxN = tb.maxN; p->maxCN = tb.maxCN; p->sumKfine = tb.sumKfine;
}

void fill_dev_problem(frx_problem *p) {
    const frx_config *cfg = &p->cfg;
    frx::DevProblem &d = p->dp;
    d.B = p->B; d.P = p->P; d.kappa = cfg->qd_intervals; d.inv_kappa = 1.0 / cfg->qd_intervals; d.soft = p->softT ? 1 : 0; d.c2 = cfg->c2_diffeo ? 1 : 0;
    d.rho = p->softT ? cfg->rho : 0.0;                                   // CPU.hpp:1098-1107
    d.sumT = p->softT ? 1.0 : cfg->total_t;
    d.pc.ell[0] = cfg->horiz_half_len; d.pc.ell[1] = cfg->horiz_half_len; d.pc.ell[2] = cfg->vert_half_len;
    d.pc.safeMargin = cfg->safe_margin;
    d.pc.vMaxSqr = cfg->vel_max * cfg->vel_max;
    d.pc.thrMinSqr = cfg->thr_acc_min * cfg->thr_acc_min;
    d.pc.thrMaxSqr = cfg->thr_acc_max * cfg->thr_acc_max;
    d.pc.bdrMaxSqr = cfg->body_rate_max * cfg->body_rate_max;
    d.pc.gAcc = cfg->grav_acc;
    for (int q = 0; q < 4; q++) d.pc.chi[q] = cfg->penalty_pvtb[q];
    d.cvoff = p->d_cvoff.p; d.poff = p->d_poff.p; d.coff = p->d_coff.p; d.xoff = p->d_xoff.p; d.boff = p->d_boff.p;
    d.headPVA = p->d_head.p; d.tailPVA = p->d_tail.p;
    d.piece_hbeg = p->d_piece_hbeg.p; d.piece_K = p->d_piece_K.p; d.piece_coarse = p->d_piece_coarse.p; d.piece_iv = p->d_piece_iv.p;
    d.coarse_iv = p->d_coarse_iv.p; d.coarse_fbeg = p->d_coarse_fbeg.p;
    d.wp_vbeg = p->d_wp_vbeg.p; d.wp_nv = p->d_wp_nv.p; d.wp_xbeg = p->d_wp_xbeg.p;
    d.hblk = p->d_hblk.p; d.vrec = p->d_vrec.p; d.wq_glob = p->d_wq.p; d.stamps = nullptr; d.cand_active = nullptr; d.piece_active = nullptr;
}

// (the first evaluation may be captured: the device copy of its arguments is complete before create returns)
hipError_t upload_eval_cluster_args(frx_problem *p) {
    if (!p->eval_fused_G) return hipSuccess;
    frx::eval_cluster_args(p->dp, p->geo, p->d_T.p, p->d_C.p, p->d_ev_ll.p, p->d_ev_words, p->d_ev_front.p, p->ev_args.data());
    return hipMemcpy(p->d_ev_args.p, p->ev_args.data(), p->ev_args.size(), hipMemcpyHostToDevice);
}

} // namespace

extern "C" {

int frx_version(void) { return FRX_VERSION; }
const char *frx_last_error(void) { return g_err.c_str(); }
int frx_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}
void frx_lbfgs_default_params(frx_lbfgs_params *p) { if (p) frx::lbfgs_defaults(*p); }
void frx_lbfgs_gcopter_params(frx_lbfgs_params *p, double rel_cost_tol) {
    if (!p) return;
    frx::lbfgs_defaults(*p);
    p->mem_size = 128; p->past = 3; p->g_epsilon = 1.0e-16; p->min_step = 1.0e-32; p->delta = rel_cost_tol;
}

int frx_problem_create(const frx_config *cfg, int device, int B, const int *coarse_n, const double *ini_state,
                       const double *fin_state, const int *h_off, const double *h_rec, const int *v_off, const double *v_rec,
                       frx_problem **out) {
    if (!cfg || !coarse_n || !ini_state || !fin_state || !h_off || !h_rec || !v_off || !v_rec || !out || B <= 0)
        return fail(FRX_ERR_INVALID_ARG, "frx_problem_create: null argument or B <= 0");
    if (cfg->qd_intervals < 1) return fail(FRX_ERR_INVALID_ARG, "qd_intervals must be >= 1");
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return frx::no_device();
    if (device < 0 || device >= ndev) return fail(FRX_ERR_INVALID_ARG, "device ordinal out of range");
    if (hipSetDevice(device) != hipSuccess) return fail(FRX_ERR_NO_DEVICE, "hipSetDevice failed");

    const auto t_create0 = clk::now();
    HandleOwner own(new (std::nothrow) frx_problem());
    frx_problem *p = own.p;
    if (!p) return fail(FRX_ERR_ALLOC, "out of host memory");
    p->cfg = *cfg;
    p->device = device;
    p->B = B;
    p->softT = cfg->rho > 0;                                             // CPU.hpp:1097
    const frx::CreateSwitches sw = create_switches_from_env();

    frx::ProblemTables tb;
    if (const int rc = create_tables(p, coarse_n, ini_state, fin_state, h_off, h_rec, v_off, v_rec, tb)) return rc;
    if (const int rc = create_geometry(p, tb, sw, ndev)) return rc;
    const double ms_host_build = ms_since(t_create0);

    hipError_t e;
    if ((e = create_stream_and_limits(p))) return create_hip_error(e, "stream and LDS limits");
    if ((e = upload_tables(p, tb))) return create_hip_error(e, "upload of the descriptor tables");
    if ((e = allocate_work_space(p, tb))) return create_hip_error(e, "device work space");
    if ((e = allocate_eval_cluster(p, tb))) return create_hip_error(e, "buffers of the one-launch evaluation");
    if ((e = allocate_staging(p, tb))) return create_hip_error(e, "pinned staging buffers");
    adopt_tables(p, tb);
    fill_dev_problem(p);
    if ((e = upload_eval_cluster_args(p))) return create_hip_error(e, "upload of the evaluation arguments");
    if (sw.setup_timing) fprintf(stderr, "[frx setup] frx_problem_create: B = %d, host descriptors %.3f ms, device allocations + uploads %.3f ms\n", B, ms_host_build, ms_since(t_create0) - ms_host_build);
    *out = own.release();
    return FRX_OK;
}

void frx_problem_destroy(frx_problem *p) {
    if (!p) return;
    (void)hipSetDevice(p->device);
    if (p->stream) { (void)hipStreamSynchronize(p->stream); (void)hipStreamDestroy(p->stream); }
    delete p;
}

// The inner boundary on its own (include/frx.h): what cuda_computer::compute receives per call (cc.cuh:118-134) - idxHs, cfgHs, the ellipsoid, margin, limits
// and weights - is everything the penalty integrator needs; the waypoint polytopes, end states and variables of the outer boundary do not exist on that side
// of the reference (MINCO_S3 knows none of them).  The handle is an ordinary one whose candidates have one coarse piece per fine piece (gridRes = inf) and
// two-vertex placeholder polytopes that no entry point of a penalty-only handle ever reads.
int frx_penalty_problem_create(const frx_config *cfg, int device, int B, const int *piece_n, const int *piece_poly, const int *h_off, const double *h_rec,
                               frx_problem **out) {
    if (!cfg || !piece_n || !piece_poly || !h_off || !h_rec || !out || B <= 0) return fail(FRX_ERR_INVALID_ARG, "frx_penalty_problem_create: null argument or B <= 0");
    *out = nullptr;
    size_t P = 0;
    for (int b = 0; b < B; b++) { if (piece_n[b] < 1) return fail(FRX_ERR_INVALID_ARG, "piece_n[b] < 1"); P += (size_t)piece_n[b]; }
    std::vector<int> hoff2(P + 1, 0), voff(1, 0);
    std::vector<double> hrec2, vrec, states((size_t)9 * B, 0.0);
    for (size_t gp = 0; gp < P; gp++) {
        const int m = piece_poly[gp];
        if (m < 0) return fail(FRX_ERR_INVALID_ARG, "piece_poly: negative polytope index");
        const int hb = h_off[m], K = h_off[m + 1] - hb;
        if (K < 1) return fail(FRX_ERR_INVALID_ARG, "an H-polytope has no half-spaces");
        hrec2.insert(hrec2.end(), h_rec + 6 * (size_t)hb, h_rec + 6 * (size_t)(hb + K));
        hoff2[gp + 1] = hoff2[gp] + K;
    }
    for (int b = 0; b < B; b++)
        for (int q = 0; q < 2 * piece_n[b] - 1; q++) {
            const double v2[6] = {0.0, 0.0, 0.0, 1.0, 0.0, 0.0};
            vrec.insert(vrec.end(), v2, v2 + 6);
            voff.push_back(voff.back() + 2);
        }
    frx_config c2 = *cfg;
    c2.grid_res = INFINITY;                                                 // one fine piece per polytope entry: idxHs is already expanded
    if (!(c2.rho > 0.0)) { c2.rho = 1.0; }                                  // (soft total time: the time layer is never evaluated on this handle, and it needs no TotalT)
    frx_problem *p = nullptr;
    const int rc = frx_problem_create(&c2, device, B, piece_n, states.data(), states.data(), hoff2.data(), hrec2.data(), voff.data(), vrec.data(), &p);
    if (rc != FRX_OK) return rc;
    p->penalty_only = true;
    *out = p;
    return FRX_OK;
}

int frx_problem_set_lbfgs_mode(frx_problem *p, int mode) {
    if (!p) return fail(FRX_ERR_INVALID_ARG, "null argument");
    if (mode != FRX_LBFGS_DEVICE_VECTORS && mode != FRX_LBFGS_HOST_VECTORS) return fail(FRX_ERR_INVALID_ARG, "unknown L-BFGS mode");
    p->lbfgs_mode = mode;
    return FRX_OK;
}

int frx_problem_set_solver(frx_problem *p, int solver) {
    if (!p) return fail(FRX_ERR_INVALID_ARG, "null argument");
    if (solver != FRX_SOLVER_KNOT_PCR && solver != FRX_SOLVER_BANDED_LU) return fail(FRX_ERR_INVALID_ARG, "unknown solver id");
    if (solver == FRX_SOLVER_BANDED_LU && !p->banded_ok)
        return fail(FRX_ERR_CAPACITY, "banded-LU kernels need the 6N x 13 band in LDS: too many pieces");
    p->geo.solver = solver;
    return FRX_OK;
}

// Diagnostic: one evaluation at x with s_memtime stamps at the phase boundaries of candidate 0's k_forward_knot
// (slots 0..6) and k_backward_knot (slots 16..24); out32 receives the raw shader-clock stamps.
int frx_profile_phases(frx_problem *p, const double *x, long long *out32) {
    if (!p || !x || !out32) return fail(FRX_ERR_INVALID_ARG, "null argument");
    HIP_TRY(hipSetDevice(p->device));
    if (!p->d_stamps.p) HIP_TRY(p->d_stamps.alloc(FRX_STAMP_SLOTS));
    HIP_TRY(hipMemset(p->d_stamps.p, 0, 64 * sizeof(long long)));
    std::vector<double> f(p->B), g(p->NX);
    int rc = frx_objective_eval(p, x, f.data(), g.data());          // warm
    if (rc != FRX_OK) return rc;
    p->dp.stamps = p->d_stamps.p;
    rc = frx_objective_eval(p, x, f.data(), g.data());
    p->dp.stamps = nullptr;
    if (rc != FRX_OK) return rc;
    HIP_TRY(hipMemcpy(out32, p->d_stamps.p, 32 * sizeof(long long), hipMemcpyDeviceToHost));
    return FRX_OK;
}

// Diagnostic: one evaluation at x in the one-launch form with cycle stamps of cluster 0 (forward map 0..12 and adjoint 16..31 as frx_profile_phases; 40..43 the leader's entry,
// end of the forward map, end of the adjoint, end; 44..48 wave 0 of the first member: entry, gate seen, granules staged, samples done, partials out).
static int profile_eval_cluster(frx_problem *p, const double *x, long long *out, int first, int n) {
    if (!p || !x || !out) return fail(FRX_ERR_INVALID_ARG, "null argument");
    if (!p->eval_fused) return fail(FRX_ERR_INVALID_ARG, "the one-launch evaluation does not apply to this handle");
    HIP_TRY(hipSetDevice(p->device));
    if (!p->d_stamps.p) HIP_TRY(p->d_stamps.alloc(FRX_STAMP_SLOTS));
    HIP_TRY(hipMemset(p->d_stamps.p, 0, FRX_STAMP_SLOTS * sizeof(long long)));
    std::vector<double> f(p->B), g(p->NX);
    int rc = frx_objective_eval(p, x, f.data(), g.data());          // warm
    if (rc != FRX_OK) return rc;
    p->dp.stamps = p->d_stamps.p; p->eval_fused_stamps = 1;
    {   // the argument block with the stamps pointer: a device copy of its own, uploaded here (a blocking call), so that no evaluation ever has to
        p->ev_args_st.assign(frx::eval_cluster_args_bytes(), 0);
        frx::eval_cluster_args(p->dp, p->geo, p->d_T.p, p->d_C.p, p->d_ev_ll.p, p->d_ev_words, p->d_ev_front.p, p->ev_args_st.data());
        hipError_t e_ = p->d_ev_args_st.p ? hipSuccess : p->d_ev_args_st.alloc(p->ev_args_st.size());
        if (e_ == hipSuccess) e_ = hipMemcpy(p->d_ev_args_st.p, p->ev_args_st.data(), p->ev_args_st.size(), hipMemcpyHostToDevice);
        if (e_ != hipSuccess) { p->dp.stamps = nullptr; p->eval_fused_stamps = 0; return fail(FRX_ERR_HIP, hipGetErrorString(e_)); }
    }
    rc = frx_objective_eval(p, x, f.data(), g.data());
    p->dp.stamps = nullptr; p->eval_fused_stamps = 0;
    if (rc != FRX_OK) return rc;
    HIP_TRY(hipMemcpy(out, p->d_stamps.p + first, n * sizeof(long long), hipMemcpyDeviceToHost));
    return FRX_OK;
}
int frx_debug_profile_eval_cluster(frx_problem *p, const double *x, long long *out64) { return profile_eval_cluster(p, x, out64, 0, 64); }
// The same evaluation with the stamps of its tail behind the first 64: out80[64..68] = wave 0 behind the barrier that follows the knot adjoint, wave 0's last gradient
// store issued, axis wave 1's last store issued, thread 0 has the verdict, thread 0 has issued `done` (100 MHz counter, as 40..48).
// out80[69..76]: the hand-off of the penalty partials (frx_debug.h; EvalHandoff, frx_kernels.hpp).
int frx_debug_profile_eval_tail(frx_problem *p, const double *x, long long *out80) { return profile_eval_cluster(p, x, out80, 0, 80); }
// And with the stamps of the forward map's prelude behind those: out112[80..84] wave 0 of the leader, [88..92] wave 0 of the last member with a task, [96..110] axis wave 1 of
// the leader (frx_debug.h; forward_knot_body<.., ET>, frx_kernels.hpp).
int frx_debug_profile_eval_forward(frx_problem *p, const double *x, long long *out112) { static_assert(FRX_STAMP_SLOTS == 112, "out112"); return profile_eval_cluster(p, x, out112, 0, FRX_STAMP_SLOTS); }

// Diagnostic (tests, tuning): drives k_lbfgs_pre alone.  `iters` successive accepted steps on random (x, g) sequences of
// length n for B candidates; after each the device search direction is compared with a plain host two-loop recursion over
// the same history (lbfgs.hpp:1381-1411, in the reference's order).  Returns the worst relative error (max-norm) and the
// mean duration in us of the last min(iters, 32) launches.  geom4 = {E, W, PF, BLK} or null for the default choice.
int frx_dv_selftest(int device, int n, int B, int m, int iters, const int *geom4, unsigned seed, double *max_rel_err, double *avg_us) {
    if (n < 1 || B < 1 || m < 1 || m > 512 || iters < 1 || !max_rel_err || !avg_us) return fail(FRX_ERR_INVALID_ARG, "bad selftest argument");
    HIP_TRY(hipSetDevice(device));
    int E = 0, W = 0, PF = 0, BLK = 4;
    frx::dv_geometry(n, &E, &W, &PF);
    if (geom4) { E = geom4[0]; W = geom4[1]; PF = geom4[2]; BLK = geom4[3]; }
    if (E == 0 || n > 64 * W * E) return fail(FRX_ERR_CAPACITY, "vector too long for k_lbfgs_pre");
    const size_t HS = frx::dv_row_stride(n, E, W, !frx::env_off("FRX_DV_TIGHT")), NX = (size_t)n * B;   // (read per call: the A/B of the row stride runs both in one process)
    DevBuf<double> dx, dg, dxp, dgp, dd, dS, dY, dys, dgt; DevBuf<int> dxoff;
    PinBuf<frx::DvCommand> cmd; PinBuf<frx::DvResult> res;
    hipError_t e;
    if ((e = dx.alloc(NX)) || (e = dg.alloc(NX)) || (e = dxp.alloc(NX)) || (e = dgp.alloc(NX)) || (e = dd.alloc(NX)) || (e = dS.alloc(m * B * HS)) ||
        (e = dY.alloc(m * B * HS)) || (e = dys.alloc((size_t)B * m)) || (e = dgt.alloc((size_t)B * m * 4)) || (e = dxoff.alloc(B + 1)) || (e = cmd.alloc(B)) || (e = res.alloc(B)))
        return fail(FRX_ERR_ALLOC, hipGetErrorString(e));
    HIP_TRY(hipMemset(dS.p, 0, sizeof(double) * m * B * HS)); HIP_TRY(hipMemset(dY.p, 0, sizeof(double) * m * B * HS));
    HIP_TRY(hipMemset(dys.p, 0, sizeof(double) * B * m)); HIP_TRY(hipMemset(dgt.p, 0, sizeof(double) * B * m * 4));
    std::vector<int> xoff(B + 1);
    for (int b = 0; b <= B; b++) xoff[b] = b * n;
    HIP_TRY(hipMemcpy(dxoff.p, xoff.data(), sizeof(int) * (B + 1), hipMemcpyHostToDevice));
    frx::DvLaunch dv;
    dv.xoff = dxoff.p; dv.x = dx.p; dv.g = dg.p; dv.xp = dxp.p; dv.gp = dgp.p; dv.d = dd.p; dv.S = dS.p; dv.Y = dY.p; dv.ys = dys.p; dv.gt = dgt.p;
    dv.ld = NX; dv.hs = HS; dv.m = m; dv.B = B; dv.E = E; dv.W = W; dv.PF = PF; dv.BLK = BLK;
    unsigned long long st = 0x9E3779B97F4A7C15ull * (seed + 1);
    auto rnd = [&]() { st += 0x9E3779B97F4A7C15ull; unsigned long long z = st; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; z ^= z >> 31; return (double)(z >> 11) * (1.0 / 9007199254740992.0) - 0.5; };
    std::vector<double> x(NX), g(NX), xp(NX), gp(NX), dref(n), ddev(NX);
    std::vector<std::vector<double>> S(B * (size_t)m, std::vector<double>(n)), Y(B * (size_t)m, std::vector<double>(n));
    std::vector<double> ysv((size_t)B * m), alpha(m);
    for (size_t i = 0; i < NX; i++) { x[i] = rnd(); g[i] = rnd(); }
    HIP_TRY(hipMemcpy(dx.p, x.data(), sizeof(double) * NX, hipMemcpyHostToDevice)); HIP_TRY(hipMemcpy(dg.p, g.data(), sizeof(double) * NX, hipMemcpyHostToDevice));
    for (int b = 0; b < B; b++) { cmd.p[b].flags = frx::DV_INIT; cmd.p[b].slot = cmd.p[b].bound = cmd.p[b].newest = 0; cmd.p[b].step = 0.0; }
    if (frx::launch_lbfgs_pre(dv, cmd.p, res.p, nullptr)) return fail(FRX_ERR_HIP, "k_lbfgs_pre launch (geometry not instantiated?)");
    HIP_TRY(hipDeviceSynchronize());
    xp = x; gp = g;
    HipEventPair evp; HIP_TRY(evp.create());
    const hipEvent_t e0 = evp.e0, e1 = evp.e1;
    double worst = 0.0, us_sum = 0.0; int us_n = 0, end = 0;
    for (int k = 1; k <= iters; k++) {
        // the new accepted point: x moves by a random step that correlates with the gradient change, so y.s > 0 mostly
        for (size_t i = 0; i < NX; i++) { const double sx = 0.1 * rnd(); x[i] = xp[i] + sx; g[i] = gp[i] + 3.0 * sx + 0.05 * rnd(); }
        HIP_TRY(hipMemcpy(dx.p, x.data(), sizeof(double) * NX, hipMemcpyHostToDevice)); HIP_TRY(hipMemcpy(dg.p, g.data(), sizeof(double) * NX, hipMemcpyHostToDevice));
        const int bound = m <= k ? m : k;
        for (int b = 0; b < B; b++) { cmd.p[b].flags = frx::DV_ADVANCE; cmd.p[b].slot = end; cmd.p[b].bound = bound; cmd.p[b].newest = end; cmd.p[b].step = 0.0; }
        HIP_TRY(hipEventRecord(e0, nullptr));
        if (frx::launch_lbfgs_pre(dv, cmd.p, res.p, nullptr)) return fail(FRX_ERR_HIP, "k_lbfgs_pre launch");
        HIP_TRY(hipEventRecord(e1, nullptr));
        HIP_TRY(hipDeviceSynchronize());
        float ms = 0.f; HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
        if (k > iters - 32) { us_sum += 1e3 * ms; us_n++; }
        HIP_TRY(hipMemcpy(ddev.data(), dd.p, sizeof(double) * NX, hipMemcpyDeviceToHost));
        for (int b = 0; b < B; b++) {
            double *sx = S[(size_t)b * m + end].data(), *yx = Y[(size_t)b * m + end].data();
            double ys = 0.0, yy = 0.0;
            for (int i = 0; i < n; i++) { sx[i] = x[b * (size_t)n + i] - xp[b * (size_t)n + i]; yx[i] = g[b * (size_t)n + i] - gp[b * (size_t)n + i]; ys += yx[i] * sx[i]; yy += yx[i] * yx[i]; }
            ysv[(size_t)b * m + end] = ys;
            for (int i = 0; i < n; i++) dref[i] = -g[b * (size_t)n + i];
            int j = (end + 1) % m;
            for (int i = 0; i < bound; i++) {
                j = (j + m - 1) % m;
                const double *sj = S[(size_t)b * m + j].data(), *yj = Y[(size_t)b * m + j].data();
                double a = 0.0; for (int q = 0; q < n; q++) a += sj[q] * dref[q];
                a /= ysv[(size_t)b * m + j]; alpha[j] = a;
                for (int q = 0; q < n; q++) dref[q] -= a * yj[q];
            }
            for (int q = 0; q < n; q++) dref[q] *= ys / yy;
            for (int i = 0; i < bound; i++) {
                const double *sj = S[(size_t)b * m + j].data(), *yj = Y[(size_t)b * m + j].data();
                double be = 0.0; for (int q = 0; q < n; q++) be += yj[q] * dref[q];
                be /= ysv[(size_t)b * m + j];
                for (int q = 0; q < n; q++) dref[q] += (alpha[j] - be) * sj[q];
                j = (j + 1) % m;
            }
            double num = 0.0, den = 0.0, dgr = 0.0;
            for (int q = 0; q < n; q++) { num = std::max(num, std::fabs(dref[q] - ddev[b * (size_t)n + q])); den = std::max(den, std::fabs(dref[q])); dgr += dref[q] * g[b * (size_t)n + q]; }
            worst = std::max(worst, num / den);
            worst = std::max(worst, std::fabs(res.p[b].dginit - dgr) / std::max(std::fabs(dgr), 1e-300));
        }
        xp = x; gp = g; end = (end + 1) % m;
    }
    *max_rel_err = worst; *avg_us = us_n ? us_sum / us_n : 0.0;
    return FRX_OK;
}

// Diagnostic (tests): the geometry and the row stride a plan whose longest vector has n_max elements runs k_lbfgs_pre with - dv_geometry and
// dv_row_stride themselves.  No device needed.
int frx_debug_dv_layout(int n_max, const int *geom4, int tight, int *out5) {
    if (n_max < 1 || !out5) return fail(FRX_ERR_INVALID_ARG, "bad layout argument");
    int E = 0, W = 0, PF = 0, BLK = 4;
    frx::dv_geometry(n_max, &E, &W, &PF);
    if (geom4) { E = geom4[0]; W = geom4[1]; PF = geom4[2]; BLK = geom4[3]; }
    if (E < 2 || E > 8 || (E & 1) || W < 1 || W > 8 || PF < 1 || PF > 16 || BLK < 1 || BLK > 4 || n_max > 64 * W * E)
        return fail(FRX_ERR_CAPACITY, "vector too long for k_lbfgs_pre (or no such geometry)");
    out5[0] = E; out5[1] = W; out5[2] = PF; out5[3] = BLK; out5[4] = (int)frx::dv_row_stride(n_max, E, W, tight != 0);
    return FRX_OK;
}

// Diagnostic (tests): ONE round of the device-vector L-BFGS on state the caller owns - upload, k_lbfgs_pre through launch_lbfgs_pre, k_lbfgs_post when f is
// given, synchronise, copy everything back.  Every array travels in its whole given length (lens7), so what lies behind the part the kernels own comes back
// as it went.  Nothing is computed here; the checks below only keep a launch inside the arrays.
int frx_debug_dv_round(int device, int B, int m, const int *geom4, int hs, const long long *lens7, const int *xoff, double *x, double *g, double *xp, double *gp,
                       double *d, double *S, double *Y, double *ys, double *gt, const void *cmd, void *res, const int *poff, int *dflags, int *pflags,
                       const double *f) {
    if (B < 1 || m < 1 || m > 512 || !geom4 || !lens7 || !xoff || !x || !g || !xp || !gp || !d || !S || !Y || !ys || !gt || !cmd || !res)
        return fail(FRX_ERR_INVALID_ARG, "bad dv round argument");
    const int E = geom4[0], W = geom4[1], PF = geom4[2], BLK = geom4[3];
    // (the same range as frx_debug_dv_layout; whether (E, W, PF, BLK) is instantiated is launch_lbfgs_pre's to say, before anything is launched.  m <= 512 and PF <= 16
    // keep the kernel's tables of 512 + 2 * 16 ages; hs below is one of the two EVEN strides the library itself takes for this batch)
    if (E < 2 || E > 8 || (E & 1) || W < 1 || W > 8 || PF < 1 || PF > 16 || BLK < 1 || BLK > 4) return fail(FRX_ERR_INVALID_ARG, "no such k_lbfgs_pre geometry");
    const long long n_vec = lens7[0], n_hist = lens7[1], n_ys = lens7[2], n_gt = lens7[3], n_df = lens7[4], n_pf = lens7[5], n_res = lens7[6];
    int n_max = 0;
    if (xoff[0] < 0) return fail(FRX_ERR_INVALID_ARG, "xoff[0] < 0");
    for (int b = 0; b < B; b++) {
        if (xoff[b + 1] <= xoff[b]) return fail(FRX_ERR_INVALID_ARG, "every candidate needs at least one variable");
        n_max = std::max(n_max, xoff[b + 1] - xoff[b]);
    }
    if (n_max > 64 * W * E) return fail(FRX_ERR_CAPACITY, "vector too long for the geometry");
    if ((size_t)hs != frx::dv_row_stride(n_max, E, W, true) && hs != 64 * W * E) return fail(FRX_ERR_INVALID_ARG, "hs is neither the tight nor the full row of this batch");
    if (xoff[B] > n_vec || (long long)B * m * hs > n_hist || (long long)B * m > n_ys || (long long)B * m * 4 > n_gt || n_res < B)
        return fail(FRX_ERR_INVALID_ARG, "an array is shorter than the batch needs");
    const frx::DvCommand *hc = (const frx::DvCommand *)cmd;
    for (int b = 0; b < B; b++)
        if ((hc[b].flags & frx::DV_ADVANCE) && (hc[b].slot < 0 || hc[b].slot >= m || hc[b].bound < 1 || hc[b].bound > m))
            return fail(FRX_ERR_INVALID_ARG, "ADVANCE command with slot or bound outside the history");
    if (dflags && n_df < B) return fail(FRX_ERR_INVALID_ARG, "dflags shorter than the batch");
    if ((pflags != nullptr) != (poff != nullptr)) return fail(FRX_ERR_INVALID_ARG, "pflags and poff come together");
    if (pflags) {
        if (poff[0] < 0 || poff[B] > n_pf) return fail(FRX_ERR_INVALID_ARG, "pflags shorter than poff asks for");
        for (int b = 0; b < B; b++) if (poff[b + 1] < poff[b]) return fail(FRX_ERR_INVALID_ARG, "poff not ascending");
    }
    HIP_TRY(hipSetDevice(device));
    DevBuf<double> dx, dg, dxp, dgp, dd, dS, dY, dys, dgt, df; DevBuf<int> dxoff, dpoff, ddf, dpf;
    PinBuf<frx::DvCommand> pc; PinBuf<frx::DvResult> pr;
    hipError_t e;
    if ((e = dx.alloc(n_vec)) || (e = dg.alloc(n_vec)) || (e = dxp.alloc(n_vec)) || (e = dgp.alloc(n_vec)) || (e = dd.alloc(n_vec)) || (e = dS.alloc(n_hist)) ||
        (e = dY.alloc(n_hist)) || (e = dys.alloc(n_ys)) || (e = dgt.alloc(n_gt)) || (e = dxoff.alloc(B + 1)) || (e = pc.alloc(B)) || (e = pr.alloc(n_res)) ||
        (dflags && (e = ddf.alloc(n_df))) || (pflags && ((e = dpf.alloc(n_pf)) || (e = dpoff.alloc(B + 1)))) || (f && (e = df.alloc(B))))
        return fail(FRX_ERR_ALLOC, hipGetErrorString(e));
    auto up = [](auto &buf, const void *h, long long count) { return count > 0 ? hipMemcpy(buf.p, h, sizeof(*buf.p) * count, hipMemcpyHostToDevice) : hipSuccess; };
    auto down = [](void *h, auto &buf, long long count) { return count > 0 ? hipMemcpy(h, buf.p, sizeof(*buf.p) * count, hipMemcpyDeviceToHost) : hipSuccess; };
    HIP_TRY(up(dx, x, n_vec)); HIP_TRY(up(dg, g, n_vec)); HIP_TRY(up(dxp, xp, n_vec)); HIP_TRY(up(dgp, gp, n_vec)); HIP_TRY(up(dd, d, n_vec));
    HIP_TRY(up(dS, S, n_hist)); HIP_TRY(up(dY, Y, n_hist)); HIP_TRY(up(dys, ys, n_ys)); HIP_TRY(up(dgt, gt, n_gt)); HIP_TRY(up(dxoff, xoff, B + 1));
    if (dflags) HIP_TRY(up(ddf, dflags, n_df));
    if (pflags) { HIP_TRY(up(dpf, pflags, n_pf)); HIP_TRY(up(dpoff, poff, B + 1)); }
    if (f) HIP_TRY(up(df, f, B));
    std::memcpy(pc.p, cmd, sizeof(frx::DvCommand) * B); std::memcpy(pr.p, res, sizeof(frx::DvResult) * n_res);
    frx::DvLaunch dv;
    dv.xoff = dxoff.p; dv.x = dx.p; dv.g = dg.p; dv.xp = dxp.p; dv.gp = dgp.p; dv.d = dd.p; dv.S = dS.p; dv.Y = dY.p; dv.ys = dys.p; dv.gt = dgt.p;
    dv.dflags = dflags ? ddf.p : nullptr; dv.pflags = pflags ? dpf.p : nullptr; dv.poff = pflags ? dpoff.p : nullptr;
    dv.ld = (size_t)n_vec; dv.hs = (size_t)hs; dv.m = m; dv.B = B; dv.E = E; dv.W = W; dv.PF = PF; dv.BLK = BLK;
    if (frx::launch_lbfgs_pre(dv, pc.p, pr.p, nullptr)) return fail(FRX_ERR_HIP, "k_lbfgs_pre launch (geometry not instantiated?)");
    if (f && frx::launch_lbfgs_post(dv, df.p, pc.p, pr.p, nullptr)) return fail(FRX_ERR_HIP, "k_lbfgs_post launch");
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(down(x, dx, n_vec)); HIP_TRY(down(g, dg, n_vec)); HIP_TRY(down(xp, dxp, n_vec)); HIP_TRY(down(gp, dgp, n_vec)); HIP_TRY(down(d, dd, n_vec));
    HIP_TRY(down(S, dS, n_hist)); HIP_TRY(down(Y, dY, n_hist)); HIP_TRY(down(ys, dys, n_ys)); HIP_TRY(down(gt, dgt, n_gt));
    if (dflags) HIP_TRY(down(dflags, ddf, n_df));
    if (pflags) HIP_TRY(down(pflags, dpf, n_pf));
    std::memcpy(res, pr.p, sizeof(frx::DvResult) * n_res);
    return FRX_OK;
}

// Diagnostic (bench): average duration of each stage kernel of an evaluation at x, HIP events on the handle's stream around `reps`
// back-to-back launches of ONE kernel at a time (the other stages run once before, so every kernel sees valid inputs).
int frx_eval_stage_times(frx_problem *p, const double *x, int reps, double *out3_us) {
    if (!p || !x || !out3_us || reps < 1) return fail(FRX_ERR_INVALID_ARG, "null argument or reps < 1");
    HIP_TRY(hipSetDevice(p->device));
    std::vector<double> f(p->B), g(p->NX);
    int rc;
    {   // (the stage kernels, not the one-launch form: their buffers are what the timed launches below read)
        struct Stage { frx_problem *q; int was, was_solo; ~Stage() { q->eval_fused = was; q->eval_solo = was_solo; } } stage{p, p->eval_fused, p->eval_solo};
        p->eval_fused = 0; p->eval_solo = 0;                             // (neither one-launch form leaves (T, C), the multipliers and the waypoint sums in global memory)
        rc = frx_objective_eval(p, x, f.data(), g.data());               // d_x, d_T, d_C, d_out20, pcrw all valid afterwards
    }
    if (rc != FRX_OK) return rc;
    HipEventPair evp; HIP_TRY(evp.create());
    const hipEvent_t e0 = evp.e0, e1 = evp.e1;
    auto time_it = [&](int which, double &us) -> int {
        for (int w = 0; w < 3; w++) {                                    // warm
            hipError_t e = hipSuccess;
            if (which == 0) e = (hipError_t)frx::launch_forward(p->dp, p->geo, p->d_x.p, p->d_T.p, p->d_C.p, p->d_band.p, p->stream);
            if (which == 1) e = (hipError_t)frx::launch_penalty(p->dp, p->geo, p->d_T.p, p->d_C.p, p->d_out20.p, p->stream);
            if (which == 2) e = (hipError_t)frx::launch_backward(p->dp, p->geo, p->d_x.p, p->d_T.p, p->d_C.p, p->d_band.p, p->d_out20.p, p->d_f.p, p->d_g.p, p->stream);
            if (e != hipSuccess) return fail(FRX_ERR_HIP, hipGetErrorString(e));
        }
        if (hipEventRecord(e0, p->stream) != hipSuccess) return fail(FRX_ERR_HIP, "hipEventRecord");
        for (int r = 0; r < reps; r++) {
            if (which == 0) (void)frx::launch_forward(p->dp, p->geo, p->d_x.p, p->d_T.p, p->d_C.p, p->d_band.p, p->stream);
            if (which == 1) (void)frx::launch_penalty(p->dp, p->geo, p->d_T.p, p->d_C.p, p->d_out20.p, p->stream);
            if (which == 2) (void)frx::launch_backward(p->dp, p->geo, p->d_x.p, p->d_T.p, p->d_C.p, p->d_band.p, p->d_out20.p, p->d_f.p, p->d_g.p, p->stream);
        }
        if (hipEventRecord(e1, p->stream) != hipSuccess || hipEventSynchronize(e1) != hipSuccess) return fail(FRX_ERR_HIP, "hipEventSynchronize");
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, e0, e1) != hipSuccess) return fail(FRX_ERR_HIP, "hipEventElapsedTime");
        us = 1e3 * ms / reps;
        return FRX_OK;
    };
    for (int k = 0; k < 3; k++) if ((rc = time_it(k, out3_us[k])) != FRX_OK) break;
    return rc;
}

// Diagnostic (bench, tests): the one-launch evaluation.  set: 1 = use it where it applies (the default), 0 = always three stage launches; returns FRX_OK.
// frx_debug_eval_fused: workgroups per candidate of the form frx_objective_eval[_device] takes right now, 0 = one launch per stage.
int frx_debug_set_eval_fused(frx_problem *p, int enable) {
    if (!p) return fail(FRX_ERR_INVALID_ARG, "null argument");
    if (enable && p->eval_fused_G && (p->eval_fused_code || (p->h_ev_status.p && *(volatile unsigned *)p->h_ev_status.p))) (void)eval_cluster_status(p, nullptr);   // a retired form comes back clean
    p->eval_fused = (enable && p->eval_fused_G) ? 1 : 0;
    p->eval_fused_ticks = enable == 2 ? 1ull : 25000000ull;               // 2 (tests): the value 1 tells the launcher to drop the members and bound the leader's waits at 50 us - the failure path
    return FRX_OK;
}
int frx_debug_eval_fused(const frx_problem *p) { return (p && p->eval_fused) ? p->eval_fused_G : 0; }
int frx_debug_eval_geometry(const frx_problem *p) { return (p && p->eval_fused) ? frx::eval_cluster_class(p->geo) : 0; }
int frx_debug_eval_front(const frx_problem *p) { return (p && p->eval_fused) ? frx::eval_cluster_front(p->geo) : 0; }
int frx_debug_eval_prelude(const frx_problem *p) { return (p && p->eval_fused) ? frx::eval_cluster_prelude(p->geo) : 0; }
int frx_debug_eval_adjoint(const frx_problem *p) { return (p && p->eval_fused) ? frx::eval_cluster_adjoint(p->geo) : 0; }
// Diagnostic (bench, tests): the solo form of an evaluation (one workgroup per candidate, one launch).  mode: 0 = never, 1 = from the handle's threshold on (the
// default), 2 = at every batch size.  frx_debug_eval_solo: workgroups of the kernel a CU holds when the NEXT evaluation of this handle takes the form, 0 = it does not.
int frx_debug_set_eval_solo(frx_problem *p, int mode) {
    if (!p || mode < 0 || mode > 2) return fail(FRX_ERR_INVALID_ARG, "null argument or unknown mode");
    if (mode == 2 && !p->geo.lds_solo) return fail(FRX_ERR_INVALID_ARG, "the solo form does not apply to this handle (more than 64 pieces or samples per piece, or the banded solver)");   // (1 = where it applies: always accepted)
    p->eval_solo = mode;
    return FRX_OK;
}
// Diagnostic (bench): which penalty kernel a stage launch of this handle takes - 0 = k_penalty (FRX_PENALTY_FORM=thr), 1 = k_penalty_lat, 2 = k_penalty_lat2 (four-wave
// workgroups, one sample per lane: the large-batch form; FRX_PENALTY_TWOPHASE=0 keeps the one-phase launch).
int frx_debug_penalty_kernel(const frx_problem *p) {
    if (!p) return -1;
    const char *f = std::getenv("FRX_PENALTY_FORM"), *tp = std::getenv("FRX_PENALTY_TWOPHASE");
    return frx::penalty_form_code(frx::penalty_form(p->geo.lds_pen2 != 0, p->geo.lpp, !f ? 0 : f[0] == 'l' ? 1 : 2, tp ? tp[0] : 0));
}
int frx_debug_eval_solo(const frx_problem *p) {
    if (!p) return 0;
    const frx::EvalRoute plain = frx::eval_route(true, false, false, false, p->eval_fused != 0, p->eval_fused_stamps != 0, p->eval_solo, p->B, p->eval_solo_min_B,
                                                 p->eval_solo_max_B, p->geo.lds_solo != 0, p->geo.solver == frx::SOLVER_KNOT_PCR);
    return plain == frx::EVAL_SOLO ? frx::eval_solo_blocks_per_cu(p->geo) : 0;
}
// Diagnostic (bench): average duration of one evaluation at x in the form frx_objective_eval_device takes, HIP events around `reps` back-to-back evaluations.
int frx_eval_launch_time(frx_problem *p, const double *x, int reps, double *out_us) {
    if (!p || !x || !out_us || reps < 1) return fail(FRX_ERR_INVALID_ARG, "null argument or reps < 1");
    HIP_TRY(hipSetDevice(p->device));
    std::vector<double> f(p->B), g(p->NX);
    int rc = frx_objective_eval(p, x, f.data(), g.data());
    if (rc != FRX_OK) return rc;
    HipEventPair evp; HIP_TRY(evp.create());
    for (int w = 0; w < 3; w++) HIP_TRY((hipError_t)launch_eval(p, p->d_x.p, p->d_f.p, p->d_g.p, p->stream, true));
    HIP_TRY(hipEventRecord(evp.e0, p->stream));
    for (int r = 0; r < reps; r++) (void)launch_eval(p, p->d_x.p, p->d_f.p, p->d_g.p, p->stream, true);
    HIP_TRY(hipEventRecord(evp.e1, p->stream));
    HIP_TRY(hipEventSynchronize(evp.e1));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, evp.e0, evp.e1));
    *out_us = 1e3 * ms / reps;
    HIP_TRY(hipMemcpy(f.data(), p->d_f.p, sizeof(double) * p->B, hipMemcpyDeviceToHost));
    return eval_cluster_status(p, f.data());
}

int frx_problem_totals(const frx_problem *p, int *out6) {
    if (!p || !out6) return fail(FRX_ERR_INVALID_ARG, "null argument");
    out6[0] = p->B; out6[1] = p->P; out6[2] = p->Pc; out6[3] = p->NX; out6[4] = p->Kmax; out6[5] = p->sumKfine;
    return FRX_OK;
}
int frx_problem_layout(const frx_problem *p, int *piece_off, int *coarse_off, int *x_off, int *dim_t) {
    if (!p) return fail(FRX_ERR_INVALID_ARG, "null argument");
    if (piece_off) std::copy(p->poff.begin(), p->poff.end(), piece_off);
    if (coarse_off) std::copy(p->coff.begin(), p->coff.end(), coarse_off);
    if (x_off) std::copy(p->xoff.begin(), p->xoff.end(), x_off);
    if (dim_t) std::copy(p->dimT.begin(), p->dimT.end(), dim_t);
    return FRX_OK;
}

int frx_initial_guess(frx_problem *p, double *x0) {
    if (!p || !x0) return fail(FRX_ERR_INVALID_ARG, "null argument");
    if (p->penalty_only) return fail(FRX_ERR_INVALID_ARG, "this handle serves frx_penalty_eval[_device] only (frx_penalty_problem_create)");
    frx::initial_guess_batch(p->cfg, p->softT, p->cand, p->xoff.data(), x0);     // one flat task list over (candidate, waypoint)
    return FRX_OK;
}

int frx_objective_eval_device(frx_problem *p, const double *x_dev, double *f_dev, double *g_dev, void *hip_stream) {
    if (!p || !x_dev || !f_dev || !g_dev) return fail(FRX_ERR_INVALID_ARG, "null argument");
    if (p->penalty_only) return fail(FRX_ERR_INVALID_ARG, "this handle serves frx_penalty_eval[_device] only (frx_penalty_problem_create)");
    HIP_TRY((hipError_t)launch_eval(p, x_dev, f_dev, g_dev, hip_stream, true));
    return FRX_OK;
}

int frx_eval_status(frx_problem *p) {
    if (!p) return fail(FRX_ERR_INVALID_ARG, "null argument");
    HIP_TRY(hipSetDevice(p->device));
    return eval_cluster_status(p, nullptr);
}

int frx_objective_eval(frx_problem *p, const double *x, double *f, double *g) {
    if (!p || !x || !f || !g) return fail(FRX_ERR_INVALID_ARG, "null argument");
    if (p->penalty_only) return fail(FRX_ERR_INVALID_ARG, "this handle serves frx_penalty_eval[_device] only (frx_penalty_problem_create)");
    HIP_TRY(hipSetDevice(p->device));
    std::memcpy(p->h_x.p, x, sizeof(double) * p->NX);
    HIP_TRY(hipMemcpyAsync(p->d_x.p, p->h_x.p, sizeof(double) * p->NX, hipMemcpyHostToDevice, p->stream));
    HIP_TRY((hipError_t)launch_eval(p, p->d_x.p, p->d_f.p, p->d_g.p, p->stream, true));
    HIP_TRY(hipMemcpyAsync(p->h_f.p, p->d_f.p, sizeof(double) * p->B, hipMemcpyDeviceToHost, p->stream));
    HIP_TRY(hipMemcpyAsync(p->h_g.p, p->d_g.p, sizeof(double) * p->NX, hipMemcpyDeviceToHost, p->stream));
    HIP_TRY(hipStreamSynchronize(p->stream));
    std::memcpy(f, p->h_f.p, sizeof(double) * p->B);
    std::memcpy(g, p->h_g.p, sizeof(double) * p->NX);
    return eval_cluster_status(p, f);
}

// Asynchronous form of frx_objective_eval for host buffers: returns once the copies and kernels are enqueued on the handle's
// stream; frx_wait() completes it and fills f, g (which must stay valid until then).  One evaluation in flight per handle.
int frx_objective_eval_async(frx_problem *p, const double *x, double *f, double *g) {
    if (!p || !x || !f || !g) return fail(FRX_ERR_INVALID_ARG, "null argument");
    if (p->penalty_only) return fail(FRX_ERR_INVALID_ARG, "this handle serves frx_penalty_eval[_device] only (frx_penalty_problem_create)");
    if (p->pending_f) return fail(FRX_ERR_INVALID_ARG, "an asynchronous evaluation is already in flight on this handle (call frx_wait)");
    HIP_TRY(hipSetDevice(p->device));
    std::memcpy(p->h_x.p, x, sizeof(double) * p->NX);
    HIP_TRY(hipMemcpyAsync(p->d_x.p, p->h_x.p, sizeof(double) * p->NX, hipMemcpyHostToDevice, p->stream));
    HIP_TRY((hipError_t)launch_eval(p, p->d_x.p, p->d_f.p, p->d_g.p, p->stream, true));
    HIP_TRY(hipMemcpyAsync(p->h_f.p, p->d_f.p, sizeof(double) * p->B, hipMemcpyDeviceToHost, p->stream));
    HIP_TRY(hipMemcpyAsync(p->h_g.p, p->d_g.p, sizeof(double) * p->NX, hipMemcpyDeviceToHost, p->stream));
    p->pending_f = f; p->pending_g = g;
    return FRX_OK;
}
int frx_wait(frx_problem *p) {
    if (!p) return fail(FRX_ERR_INVALID_ARG, "null argument");
    HIP_TRY(hipSetDevice(p->device));
    HIP_TRY(hipStreamSynchronize(p->stream));
    if (p->pending_f) {
        std::memcpy(p->pending_f, p->h_f.p, sizeof(double) * p->B);
        std::memcpy(p->pending_g, p->h_g.p, sizeof(double) * p->NX);
        const double *fdone = p->pending_f;
        p->pending_f = nullptr; p->pending_g = nullptr;
        return eval_cluster_status(p, fdone);
    }
    return FRX_OK;
}

int frx_penalty_eval_device(frx_problem *p, const double *T_dev, const double *C_dev, double *out_dev, void *hip_stream) {
    if (!p || !T_dev || !C_dev || !out_dev) return fail(FRX_ERR_INVALID_ARG, "null argument");
    HIP_TRY((hipError_t)frx::launch_penalty(p->dp, p->geo, T_dev, C_dev, out_dev, hip_stream));
    return FRX_OK;
}

// The blocking penalty takes (T, C) from the host the way the trajectory entries do (frx_traj.cpp): stage_TC, its _device entry on the handle's stream, fetch_rows
// (frx_handle.hpp), then the sum over each candidate's pieces.
int frx_penalty_eval(frx_problem *p, const double *T, const double *C, double *cost, double *gdT, double *gdC) {
    if (!p || !T || !C || !cost || !gdT || !gdC) return fail(FRX_ERR_INVALID_ARG, "null argument");
    HIP_TRY(hipSetDevice(p->device));
    FRX_TRY(stage_TC(p, T, C));
    FRX_TRY(frx_penalty_eval_device(p, p->d_T.p, p->d_C.p, p->d_out20.p, p->stream));
    FRX_TRY(fetch_rows(p, p->d_out20.p, 20 * (size_t)p->P, nullptr));
    // accumulate, like cuda_computer::compute (cc.cu:549-559)
    for (int b = 0; b < p->B; b++) {
        double s = 0.0;
        for (int gp = p->poff[b]; gp < p->poff[b + 1]; gp++) {
            const double *o = p->h_out20.p + 20 * (size_t)gp;
            s += o[0];
            gdT[gp] += o[1];
            for (int v = 0; v < 18; v++) gdC[18 * (size_t)gp + v] += o[2 + v];
        }
        cost[b] += s;
    }
    return FRX_OK;
}

int frx_forward(frx_problem *p, const double *x, double *T, double *C) {
    if (!p || !x) return fail(FRX_ERR_INVALID_ARG, "null argument");
    if (p->penalty_only) return fail(FRX_ERR_INVALID_ARG, "this handle serves frx_penalty_eval[_device] only (frx_penalty_problem_create)");
    HIP_TRY(hipSetDevice(p->device));
    std::memcpy(p->h_x.p, x, sizeof(double) * p->NX);
    HIP_TRY(hipMemcpyAsync(p->d_x.p, p->h_x.p, sizeof(double) * p->NX, hipMemcpyHostToDevice, p->stream));
    HIP_TRY((hipError_t)launch_eval(p, p->d_x.p, nullptr, nullptr, p->stream, false));
    HIP_TRY(hipMemcpyAsync(p->h_T.p, p->d_T.p, sizeof(double) * p->P, hipMemcpyDeviceToHost, p->stream));
    HIP_TRY(hipMemcpyAsync(p->h_C.p, p->d_C.p, sizeof(double) * 18 * (size_t)p->P, hipMemcpyDeviceToHost, p->stream));
    HIP_TRY(hipStreamSynchronize(p->stream));
    if (T) std::memcpy(T, p->h_T.p, sizeof(double) * p->P);
    if (C) std::memcpy(C, p->h_C.p, sizeof(double) * 18 * (size_t)p->P);
    return FRX_OK;
}

int frx_debug_shader_clock(int device, double ms, double *mhz_min, double *mhz_mean, double *mhz_max) {
    if (ms <= 0.0 || ms > 100.0) return fail(FRX_ERR_INVALID_ARG, "frx_debug_shader_clock: 0 < ms <= 100");
    HIP_TRY(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    const int blocks = std::max(1, prop.multiProcessorCount);
    DevBuf<double> out; DevBuf<unsigned long long> st;
    if (out.alloc(1) != hipSuccess || st.alloc((size_t)2 * blocks) != hipSuccess) return fail(FRX_ERR_ALLOC, "clock probe buffers");
    HIP_TRY((hipError_t)frx::launch_clock_probe(out.p, st.p, blocks, (unsigned long long)(ms * 1e5), nullptr));
    HIP_TRY(hipDeviceSynchronize());
    std::vector<unsigned long long> h((size_t)2 * blocks);
    HIP_TRY(hipMemcpy(h.data(), st.p, sizeof(unsigned long long) * h.size(), hipMemcpyDeviceToHost));
    double lo = 1e30, hi = 0.0, sum = 0.0;
    for (int b = 0; b < blocks; b++) { const double mhz = 100.0 * (double)h[2 * b] / (double)std::max<unsigned long long>(1, h[2 * b + 1]); lo = std::min(lo, mhz); hi = std::max(hi, mhz); sum += mhz; }
    if (mhz_min) *mhz_min = lo;
    if (mhz_mean) *mhz_mean = sum / blocks;
    if (mhz_max) *mhz_max = hi;
    return FRX_OK;
}
int frx_debug_lane_exchange(int device, int stride, const void *in64, void *below64, void *above64) {
    if (!in64 || !below64 || !above64) return fail(FRX_ERR_INVALID_ARG, "frx_debug_lane_exchange: null buffer");
    if (stride != 1 && stride != 2 && stride != 4 && stride != 8 && stride != 16 && stride != 32) return fail(FRX_ERR_INVALID_ARG, "frx_debug_lane_exchange: stride in {1, 2, 4, 8, 16, 32}");
    HIP_TRY(hipSetDevice(device));
    DevBuf<double> buf;
    if (buf.alloc(3 * 64) != hipSuccess) return fail(FRX_ERR_ALLOC, "lane exchange probe buffers");
    HIP_TRY(hipMemset(buf.p, 0, sizeof(double) * 3 * 64));
    HIP_TRY(hipMemcpy(buf.p, in64, sizeof(double) * 64, hipMemcpyHostToDevice));
    HIP_TRY((hipError_t)frx::launch_lane_exchange_probe(stride, buf.p, buf.p + 64, buf.p + 128, nullptr));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(below64, buf.p + 64, sizeof(double) * 64, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(above64, buf.p + 128, sizeof(double) * 64, hipMemcpyDeviceToHost));
    return FRX_OK;
}
int frx_debug_compact_from_history(int m, int n, int hs, int bound, int newest, const double *S, const double *Y, double *rinv129, double *yy, double *vd) {
    if (!S || !Y || !rinv129 || !yy || !vd || m < 1 || m > 128 || n < 1 || hs < n || bound < 0 || bound > m || newest < 0 || newest >= m) return fail(FRX_ERR_INVALID_ARG, "frx_debug_compact_from_history: argument out of range");
    frx::compact_from_history(m, n, (size_t)hs, bound, newest, S, Y, 129, rinv129, yy, vd);
    return FRX_OK;
}
} // extern "C"
