// The handle behind the C ABI (struct frx_problem) and the small HIP helpers its translation units share (device buffers: frx_hip_scope.hpp): frx_api.cpp (creation, evaluation,
// self-tests), frx_traj.cpp (the trajectory entries), frx_optimize.cpp (the plan drivers) and frx_host_cpus.cpp (CPU budget, NUMA placement).  Private to libfrx.so; host code only.
#pragma once
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <string>
#include <vector>

#include <sched.h>

#include "../../include/frx.h"
#include "frx_device.hpp"
#include "frx_eval_front.hpp"
#include "frx_hip_scope.hpp"
#include "frx_host_setup.hpp"
#include "frx_internal.hpp"
#include "frx_lbfgs.hpp"
#include "frx_plan_route.hpp"

// records the text frx_last_error() returns on this thread (one definition of the thread-local string: frx_api.cpp)
inline int fail(int code, const std::string &msg) { return frx::set_error(code, msg); }

#define HIP_TRY(expr)                                                                                   \
    do {                                                                                                \
        hipError_t e_ = (expr);                                                                         \
        if (e_ != hipSuccess)                                                                           \
            return fail(FRX_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));                \
    } while (0)
#define FRX_TRY(expr) do { const int rc_ = (expr); if (rc_ != FRX_OK) return rc_; } while (0)

// a pair of HIP events that is destroyed on every exit path
struct HipEventPair {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipError_t create() { hipError_t e = hipEventCreate(&e0); return e != hipSuccess ? e : hipEventCreate(&e1); }
    ~HipEventPair() { if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); }
};

using clk = std::chrono::steady_clock;
inline double ms_since(clk::time_point t0) { return std::chrono::duration<double, std::milli>(clk::now() - t0).count(); }

template <class T> struct PinBuf {
    T *p = nullptr;
    size_t n = 0;
    ~PinBuf() { if (p) (void)hipHostFree(p); }
    void release() { if (p) (void)hipHostFree(p); p = nullptr; n = 0; }
    hipError_t alloc(size_t count) {
        release();
        hipError_t e = hipHostMalloc((void **)&p, std::max<size_t>(count, 1) * sizeof(T), hipHostMallocMapped | hipHostMallocCoherent);
        if (e == hipSuccess) { n = count; std::memset(p, 0, std::max<size_t>(count, 1) * sizeof(T)); } else p = nullptr;
        return e;
    }
    hipError_t reserve(size_t count) { return n >= count && p ? hipSuccess : alloc(count); }   // keep what is large enough
};

namespace frx {
// frx_host_cpus.cpp
int mailbox_threads(int S);
bool device_numa_cpus(int device, cpu_set_t *out);
// The calling thread on the CPUs of the device's NUMA node for the length of a scope (FRX_NUMA=0: wherever it is).  Used around the allocation - and first touch - of
// the mailboxes in mapped host memory: pinned pages are taken from the node the allocating thread runs on, and a process whose main thread happened to sit on the other
// socket at that moment kept its mailboxes there for good - every command the device read and every result it wrote crossed the socket interconnect, and so did the
// service threads' scans from the right socket.  Round 6 found the two MODES of a process that round 5 put down to "the box's host" (profiles/r06_mode_probe.jsonl:
// 25.0-25.2 us per round with a mailbox scan of 0.07 us, 26.2-26.3 with 0.12-0.15, constant within a process, same clocks, same XCD placement; stretching the scan
// period itself to 3.2 us changes nothing, profiles/r06_ab_host_scan.jsonl).
struct NumaScope {
    cpu_set_t saved; bool active = false;
    explicit NumaScope(int device);
    ~NumaScope();
};
} // namespace frx

constexpr int FRX_STAMP_SLOTS = 112;                        // words of frx_problem::d_stamps

struct frx_problem {
    frx_config cfg;
    int device = 0, B = 0, P = 0, Pc = 0, NX = 0, Kmax = 0, maxN = 0, maxCN = 0, sumKfine = 0;
    bool softT = true;
    std::vector<frx::HostCand> cand;
    std::vector<int> poff, coff, xoff, boff, dimT;
    frx::DevProblem dp;
    hipStream_t stream = nullptr;
    // device-resident constants
    DevBuf<int> d_cvoff, d_poff, d_coff, d_xoff, d_boff, d_piece_hbeg, d_piece_K, d_piece_coarse, d_piece_iv, d_coarse_iv, d_coarse_fbeg, d_wp_vbeg,
        d_wp_nv, d_wp_xbeg;
    DevBuf<double> d_head, d_tail, d_hblk, d_vrec;
    // device work space
    DevBuf<double> d_x, d_f, d_g, d_T, d_C, d_band, d_out20;
    DevBuf<long long> d_stamps;                             // FRX_STAMP_SLOTS words (0..63 as ever; 64..79 the tail of the one-launch evaluation, frx_debug_profile_eval_tail; 80..111 its prelude, frx_debug_profile_eval_forward)
    DevBuf<double> d_pcrw;
    DevBuf<double> d_wq;                                    // [P][4]: per waypoint {|xi|^2, sum_a V_a xi_a^2}, forward map -> adjoint of the same evaluation
    // pinned staging
    PinBuf<double> h_x, h_f, h_g, h_T, h_C, h_out20;
    DevBuf<double> d_rows;                                  // [P][20]: the piece rows of the blocking frx_trajectory_check, _extrema and _contain, allocated by whichever runs first
    DevBuf<double> d_sample, d_gates, d_clear, d_mapdist;   // scratch of the blocking frx_trajectory_sample, _gates, _clearance[_exact] and _map_distance, grown as needed: carve_* (frx_traj_host.hpp) lay them out
    int clear_chunk = 0;                                    // tests (frx_debug_set_clear_chunk): > 0 = cloud points per chunk, 0 = the library's own split
    int clx_chunk = 0, clx_cull = 1;                        // tests (frx_debug_set_clear_exact): cloud points per chunk of frx_trajectory_clearance_exact (0 = the library's own split), the cull on / off
    const double *clx_last_work = nullptr; int clx_last_nchunks = 0;   // the partials of the last exact clearance call on the handle (frx_debug_clear_exact_counts reads its counts)
    // device-vector L-BFGS state (allocated on first use)
    DevBuf<double> d_xp, d_gp, d_dir, d_S, d_Y, d_ys, d_gt;
    PinBuf<frx::DvCommand> h_cmd;
    PinBuf<frx::DvResult> h_res;
    int dv_mem = 0; size_t dv_hs = 0;
    double *pending_f = nullptr, *pending_g = nullptr;      // outputs of an frx_objective_eval_async awaiting frx_wait
    // line-search tap of k_backward_knot (set only while optimize_device_vectors runs)
    frx::TapLaunch tap;
    DevBuf<unsigned> d_arrive; PinBuf<unsigned> h_flag; DevBuf<int> d_flags, d_pflags;
    // resident round kernel (frx_round_kernel.hpp): cluster exchange buffers and mapped mailboxes, allocated on first use
    DevBuf<double> d_pubsyg, d_part, d_upub, d_dpub, d_rdbg, d_out20ll;
    int dirlog_cap = 0, dirlog_cands = 0, dirlog_nxp = 0;   // direction log of the resident kernel (frx_debug_direction_log): records asked for / row geometry of the last plan
    std::vector<double> dirlog;                             // [B] counts, then dirlog_cands x dirlog_cap records of 4 NXP + 2 doubles
    DevBuf<unsigned long long> d_rprof;                     // FRX_RESIDENT_PROF: [B][G][16] per-segment ticks of the last resident launch
    std::vector<unsigned long long> rprof;
    DevBuf<unsigned> d_rwords;
    DevBuf<unsigned char> d_rargs;                          // the resident launch's arguments in device memory (k_round takes them by pointer)
    PinBuf<unsigned long long> h_rcmd, h_rres;              // [S] x 8 words each (S clusters: one mailbox per cluster)
    int rk_B = 0, rk_S = 0, rk_G = 0, rk_NXP = 0;
    // take-over of a per-stage batch's stragglers by the resident kernel (optimize_resident with a TakeOver): per cluster candidate index, last objective value,
    // newest slot and pair count of its history, and the dense state rebuilt from that history (frx_compact.hpp)
    DevBuf<int> d_rs_int; DevBuf<double> d_rs_f, d_rs_rinv, d_rs_yy, d_rs_vd;
    int taken_over = 0;                                     // candidates of the last plan that finished on the resident kernel after per-stage rounds
    long takeover_at = 0;                                   // tests (frx_debug_set_takeover_at): > 0 = every plan starts as per-stage rounds and hands over after this many, whatever the batch size
    int resident_clusters = 0;                              // clusters of the last resident launch (< B: the candidates went through the work queue)
    int resident_mode = 1;                                  // 1 = use the resident kernel when it applies (frx_problem_set_resident); 2 = also when the batch
                                                            // is larger than the chip holds at once, whatever its size (work queue); 0 = never
    int resident_retry = 0;                                 // 1 = re-run candidates that fail on the resident kernel on the per-stage rounds (diagnostic, frx_debug_set_resident_retry); the reference takes no second chance and neither does the default
    int resident_retried = 0;                               // candidates of the last plan re-run on the per-stage rounds after an L-BFGS error
    unsigned long long spec_counts[4] = {0, 0, 0, 0};       // last resident plan, summed over candidates: rounds started on a predicted ADVANCE / trial step, predictions redone, reserved
    int resident_failed = 0;                                // candidates of the last resident plan that ended with an L-BFGS error other than the iteration limit
    int resident_used = 0;                                  // diagnostics: 1 = the last frx_optimize ran on the resident kernel
    unsigned resident_status = 0;                           // device-side error code of the last resident launch (RK_ERR_*)
    std::vector<double> trace;                              // FRX_TRACE: per command of candidate 0 {flags, step, f, dg, dginit, xx, gg}
    // one launch per evaluation (frx_eval_kernel.hpp): granules and control words of its clusters, zeroed once; eval_fused: 1 = frx_objective_eval[_device] take it
    // (set at create when the geometry applies and the chip holds the whole batch at once; FRX_EVAL_FUSED=0 / frx_debug_set_eval_fused turn it off)
    DevBuf<unsigned long long> d_ev_ll; unsigned *d_ev_words = nullptr;   // one allocation: [40 P] granule words, then the [64 B + 1] control words
    int eval_fused = 0, eval_fused_G = 0, eval_fused_stamps = 0;
    unsigned long long eval_fused_ticks = 25000000ull;      // bound of every wait inside the launch, ticks of the 100 MHz counter: 250 ms (a healthy evaluation takes ~20 us; FRX_EVAL_TIMEOUT_MS)
    std::vector<unsigned char> ev_args, ev_args_st;         // the one-launch evaluation's constant arguments (frx::eval_cluster_args), host copies: without / with the stamps pointer
    DevBuf<frx::EvalFront> d_ev_front;                      // the one-launch evaluation's front records, one per candidate (frx_eval_front.hpp): constant for the handle's life, uploaded at create
    DevBuf<unsigned char> d_ev_args, d_ev_args_st;          // their device copies: uploaded at create / by the diagnostic that sets the pointer (profile_eval_cluster) - never by an evaluation
    PinBuf<unsigned> h_ev_status;                           // mapped host word: the code of an expired wait, written by the leader that saw it - launch_eval reads it without a synchronisation
    unsigned eval_fused_code = 0;                           // the code that retired the one-launch form on this handle (0: none)
    // one launch per evaluation for LARGE batches (frx_solo_kernel.hpp: one workgroup per candidate): 0 = never, 1 = from eval_solo_min_B candidates on (default), 2 = always
    int eval_solo = 0, eval_solo_min_B = 0, eval_solo_max_B = 0;
    frx::LaunchGeom geo;
    bool banded_ok = true;
    bool penalty_only = false;              // frx_penalty_problem_create: the inner boundary alone (no variables, no waypoint polytopes: only frx_penalty_eval[_device] apply)
    int lbfgs_mode = 0;                     // 0 = device vectors (default), 1 = host vectors
    frx::PlanTimes stats;                   // frx_optimize_stats: what the last plan took
};

// What the blocking entries that take (T, C) from the host share (frx_penalty_eval, frx_traj.cpp): (T, C) -> d_T, d_C through the pinned h_T, h_C on the handle's stream
inline int stage_TC(frx_problem *p, const double *T, const double *C) {
    std::memcpy(p->h_T.p, T, sizeof(double) * p->P);
    std::memcpy(p->h_C.p, C, sizeof(double) * 18 * (size_t)p->P);
    HIP_TRY(hipMemcpyAsync(p->d_T.p, p->h_T.p, sizeof(double) * p->P, hipMemcpyHostToDevice, p->stream));
    HIP_TRY(hipMemcpyAsync(p->d_C.p, p->h_C.p, sizeof(double) * 18 * (size_t)p->P, hipMemcpyHostToDevice, p->stream));
    return FRX_OK;
}
// n <= 20 P doubles of piece rows -> h_out20, complete on return; piece_out, when given, gets a copy
inline int fetch_rows(frx_problem *p, const double *d_rows, size_t n, double *piece_out) {
    HIP_TRY(hipMemcpyAsync(p->h_out20.p, d_rows, sizeof(double) * n, hipMemcpyDeviceToHost, p->stream));
    HIP_TRY(hipStreamSynchronize(p->stream));
    if (piece_out) std::memcpy(piece_out, p->h_out20.p, sizeof(double) * n);
    return FRX_OK;
}
// a scratch buffer that grows to `need` doubles
inline int grow(DevBuf<double> &buf, size_t need, const char *entry) { return buf.n < need ? dev_alloc(buf, need, entry) : FRX_OK; }

namespace frx {
// frx_api.cpp: one evaluation of the batch in the form the handle's state selects (hipError_t as int), and the one-launch form's sticky error word
int launch_eval(frx_problem *p, const double *x_dev, double *f_dev, double *g_dev, void *st, bool backward);
int eval_cluster_status(frx_problem *p, const double *f);
} // namespace frx
