// The plan drivers behind frx_optimize: host vectors (drive_batch), device vectors with one launch per stage (optimize_device_vectors), and the resident round
// kernel (optimize_resident: one launch per plan, frx_resident_plan.hpp decides its geometry, frx_resident_mailbox.hpp talks to its clusters).  Which of them a plan
// takes, the second chance of failed candidates and the take-over between the last two are decided in frx_plan_route.hpp, from the environment as read once per
// frx_optimize call (plan_switches_from_env); this file plays the drivers.  Host-only translation unit (g++), built with the CPU oracle's floating-point flags like
// the rest of the host side.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <atomic>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include <pthread.h>
#include <sched.h>

#include "../../include/frx.h"
#include "../../include/frx_debug.h"
#include "frx_handle.hpp"
#include "frx_host_pool.hpp"
#include "frx_compact.hpp"
#include "frx_plan_route.hpp"
#include "frx_resident_plan.hpp"
#include "frx_resident_mailbox.hpp"

using frx::NumaScope;

// every wait is bounded ("status codes, bounded waits"): FRX_ROUND_TIMEOUT_MS, default 5 s per round
static double round_timeout_ms() { const char *e = std::getenv("FRX_ROUND_TIMEOUT_MS"); const double v = e ? std::atof(e) : 0.0; return v > 0.0 ? v : 5000.0; }

// waits until the stream has drained, at most timeout_ms: FRX_OK, FRX_ERR_HIP (the stream's error) or FRX_ERR_TIMEOUT
static int wait_stream(hipStream_t stream, double timeout_ms, const char *what) {
    const auto tw = clk::now();
    for (unsigned spins = 1;; spins++) {
        const hipError_t q = hipStreamQuery(stream);
        if (q == hipSuccess) return FRX_OK;
        if (q != hipErrorNotReady) return fail(FRX_ERR_HIP, std::string(what) + " failed: " + hipGetErrorString(q));
        if ((spins & 0x3FF) == 0 && ms_since(tw) > timeout_ms) return fail(FRX_ERR_TIMEOUT, std::string(what) + " did not complete within its time limit (FRX_ROUND_TIMEOUT_MS)");
        __builtin_ia32_pause();
    }
}

// The batched driver shared by frx_optimize (device evaluator) and frx_lbfgs_minimize_batch (callback evaluator).
template <class EvalAll>
static int drive_batch(int count, const int *x_off, double *x, double *g, double *f, const frx_lbfgs_params &pm, int n_threads,
                       int *status, int *iters, int *evals, double *f_out, frx::PlanTimes *stats, EvalAll &&eval_all) {
    std::vector<frx::Solver> sv(count);
    frx::SpinPool pool(std::min(n_threads, count));
    // allocation + first touch of each solver's history by its owning (pinned) worker
    pool.run(count, [&](int i) { sv[i].start(x_off[i + 1] - x_off[i], x + x_off[i], g + x_off[i], pm); });
    std::vector<int> active;
    active.reserve(count);
    double t_eval = 0.0, t_host = 0.0;
    long rounds = 0;
    const auto t0 = clk::now();
    for (;;) {
        active.clear();
        for (int i = 0; i < count; i++)
            if (!sv[i].done()) active.push_back(i);
        if (active.empty()) break;
        auto te = clk::now();
        int rc = eval_all((int)active.size(), active.data());
        if (rc != FRX_OK) return rc;
        t_eval += ms_since(te);
        auto th = clk::now();
        pool.run(count, [&](int i) { if (!sv[i].done()) sv[i].feed(f[i]); });
        t_host += ms_since(th);
        rounds++;
    }
    if (stats) *stats = {ms_since(t0), t_eval, t_host, (double)rounds};
    for (int i = 0; i < count; i++) {
        if (status) status[i] = sv[i].status();
        if (iters) iters[i] = sv[i].iterations();
        if (evals) evals[i] = sv[i].evaluations();
        if (f_out) f_out[i] = sv[i].value();
    }
    return FRX_OK;
}

using frx::TakeOver;

// the environment of THIS frx_optimize call (tests and A/B runs change it between two plans of one process)
static frx::PlanSwitches plan_switches_from_env() {
    frx::PlanSwitches sw;
    sw.lbfgs_host = frx::env_is("FRX_LBFGS", 'h');
    sw.resident_off = frx::env_off("FRX_RESIDENT");
    if (const char *e = std::getenv("FRX_RESIDENT_RETRY")) sw.resident_retry = (unsigned char)e[0];
    sw.takeover_off = frx::env_off("FRX_TAKEOVER");
    sw.resident_queue_off = frx::env_off("FRX_RESIDENT_QUEUE");
    if (const char *e = std::getenv("FRX_HOST_THREADS")) { sw.host_threads_set = true; sw.host_threads = std::atoi(e); }
    sw.zero_copy = !frx::env_off("FRX_ZERO_COPY");
    sw.round_timeout_ms = round_timeout_ms();
    if (const char *e = std::getenv("FRX_DV_GEOM")) { sw.dv_geom_set = true; sw.dv_geom = e; }
    sw.dv_tight = !frx::env_off("FRX_DV_TIGHT");
    sw.mailbox = !frx::env_off("FRX_MAILBOX");
    if (const char *e = std::getenv("FRX_SKIP_INACTIVE")) sw.skip_inactive = e[0] != '0';
    if (const char *e = std::getenv("FRX_DEBUG_DROP_ROUND")) sw.drop_round = std::atol(e);
    sw.trace = std::getenv("FRX_TRACE") != nullptr;
    return sw;
}

// ---- device vectors, one launch per stage ----

// vectors, history and the command / result mailboxes of the per-stage rounds at history length m and row stride HS, the history zeroed; 1: the history does not fit
static int reserve_dv_buffers(frx_problem *p, int m, size_t HS) {
    if (p->dv_mem == m && p->dv_hs == HS) return FRX_OK;
    const int B = p->B;
    hipError_t e;
    p->dv_mem = 0; p->dv_hs = 0;
    const size_t hist = (size_t)m * B * HS;
    NumaScope numa_alloc(p->device);                                          // command / result mailboxes of the per-stage rounds: pages from the device's NUMA node
    if ((e = p->d_xp.reserve(p->NX)) != hipSuccess || (e = p->d_gp.reserve(p->NX)) != hipSuccess || (e = p->d_dir.reserve(p->NX)) != hipSuccess ||
        (e = p->d_S.reserve(hist)) != hipSuccess || (e = p->d_Y.reserve(hist)) != hipSuccess ||
        (e = p->d_ys.reserve((size_t)B * m)) != hipSuccess || (e = p->d_gt.reserve((size_t)B * m * 4)) != hipSuccess || (e = p->h_cmd.reserve(B)) != hipSuccess || (e = p->h_res.reserve(B)) != hipSuccess) {
        (void)hipGetLastError();
        if (e == hipErrorOutOfMemory) {                                       // the history does not fit: the host-vector solver needs no device history
            p->d_S.release(); p->d_Y.release();
            return 1;
        }
        return fail(FRX_ERR_ALLOC, std::string("device-vector L-BFGS buffers: ") + hipGetErrorString(e));
    }
    // zero padding of the history slices is relied upon by the unconditional 16-byte loads of k_lbfgs_pre; on the handle's
    // stream, like every consumer (the stream is non-blocking: the null stream would not order against it)
    if ((e = hipMemsetAsync(p->d_S.p, 0, sizeof(double) * hist, p->stream)) != hipSuccess || (e = hipMemsetAsync(p->d_Y.p, 0, sizeof(double) * hist, p->stream)) != hipSuccess)
        return fail(FRX_ERR_HIP, hipGetErrorString(e));
    p->dv_mem = m; p->dv_hs = HS;
    return FRX_OK;
}

// the tap, the inactive-skip flags and the mailbox are the handle's only while a per-stage plan runs: cleared on every exit
struct TapGuard { frx_problem *q; ~TapGuard() { q->tap = frx::TapLaunch(); q->dp.cand_active = nullptr; q->dp.piece_active = nullptr; } };

// With the knot/PCR kernels the reductions the line search needs ride on k_backward_knot (LineSearchTap; the banded-LU kernels keep the separate k_lbfgs_post):
// arms the tap, the flags that let the objective kernels skip inactive candidates, and (mailbox) the round's completion post in mapped memory
static int arm_tap(frx_problem *p, const frx::PlanSwitches &sw, bool mailbox, frx::DvLaunch &dv) {
    const int B = p->B;
    hipError_t e;
    if (!p->d_flags.p && (e = p->d_flags.alloc(B)) != hipSuccess) return fail(FRX_ERR_ALLOC, hipGetErrorString(e));
    dv.dflags = p->d_flags.p;
    p->tap.d = p->d_dir.p; p->tap.flags = p->d_flags.p; p->tap.res = p->h_res.p;
    if (frx::skip_inactive(sw.skip_inactive, B)) {
        if (!p->d_pflags.p && (e = p->d_pflags.alloc(p->P)) != hipSuccess) return fail(FRX_ERR_ALLOC, hipGetErrorString(e));
        dv.pflags = p->d_pflags.p; dv.poff = p->d_poff.p;
        p->dp.cand_active = p->d_flags.p; p->dp.piece_active = p->d_pflags.p;
    }
    if (!mailbox) return FRX_OK;
    NumaScope numa_alloc(p->device);
    if (!p->d_arrive.p && ((e = p->d_arrive.alloc(1)) != hipSuccess || (e = p->h_flag.alloc(1)) != hipSuccess)) return fail(FRX_ERR_ALLOC, hipGetErrorString(e));
    HIP_TRY(hipMemsetAsync(p->d_arrive.p, 0, sizeof(unsigned), p->stream));
    p->h_flag.p[0] = 0;
    p->tap.arrive = p->d_arrive.p; p->tap.flag = p->h_flag.p; p->tap.round = 0;
    return FRX_OK;
}

// Completion of a round: the last workgroup of k_backward_knot posts the round number in mapped memory (LineSearchTap).  The spin is bounded: a stream that drains
// without the post (arrival counter out of step, e.g. a launch that never happened) is reported at once, anything else after the deadline; the counters are
// re-initialised by the next plan.
static int wait_round_post(frx_problem *p, double timeout_ms) {
    const auto tw = clk::now();
    for (unsigned spins = 1;; spins++) {
        if (*(volatile unsigned *)p->h_flag.p == p->tap.round) return FRX_OK;
        if ((spins & 0x3FFF) == 0) {
            const hipError_t q = hipStreamQuery(p->stream);
            if (q == hipSuccess) {
                if (*(volatile unsigned *)p->h_flag.p == p->tap.round) return FRX_OK;
                return fail(FRX_ERR_TIMEOUT, "round " + std::to_string(p->tap.round) + ": the stream drained but completion was never posted (arrival counter out of step)");
            }
            if (q != hipErrorNotReady) return fail(FRX_ERR_HIP, std::string("device round failed: ") + hipGetErrorString(q));
            if (ms_since(tw) > timeout_ms) return fail(FRX_ERR_TIMEOUT, "round " + std::to_string(p->tap.round) + " did not complete within FRX_ROUND_TIMEOUT_MS");
        }
        __builtin_ia32_pause();
    }
}
// the end of a round: its post when there is one, else the drained stream; after an error a bounded drain, the first error kept
static int wait_round(frx_problem *p, bool posted, double timeout_ms) {
    const int rc = posted ? wait_round_post(p, timeout_ms) : wait_stream(p->stream, timeout_ms, "device round");
    if (rc == FRX_OK) return rc;
    const std::string keep = frx_last_error();
    (void)wait_stream(p->stream, timeout_ms, "device round");
    return fail(rc, keep);
}

// a per-stage plan's host state: a solver per candidate, and where every candidate's history stands on the device (for a hand-over)
struct DvPlan {
    std::vector<frx::SolverDV> sv;
    std::vector<int> newest, bound;
    std::vector<double> f_last;
    explicit DvPlan(int B) : sv(B), newest(B, 0), bound(B, 0), f_last(B, 0.0) {}
};

// the round's results to the solvers, which write their next commands (FRX_TRACE: candidate 0's row)
static void feed_round(frx_problem *p, DvPlan &pl, bool tracing) {
    for (int b = 0; b < p->B; b++) {
        frx::DvCommand &c = p->h_cmd.p[b];
        const bool evaluated = (c.flags & frx::DV_EVAL) != 0;
        if (!evaluated) { c.flags = 0; continue; }                         // a RESTORE has been executed
        if (tracing && b == 0) { const frx::DvResult &r = p->h_res.p[b]; const double row[7] = {(double)c.flags, c.step, r.f, r.dg, r.dginit, r.xx, r.gg}; p->trace.insert(p->trace.end(), row, row + 7); }
        pl.f_last[b] = p->h_res.p[b].f;
        if (pl.sv[b].saw_nonfinite(p->h_res.p[b].f)) pl.sv[b].give_up(frx::LBERR_ROUNDING); else pl.sv[b].feed(p->h_res.p[b]);
    }
}

// the plan's results from the staged x and the solvers - or, of a candidate that is handed over (take: still running), its solver, pending command and history position
static void collect_or_hand_over(const frx_problem *p, const DvPlan &pl, const std::vector<char> *only, TakeOver *take, const frx::PlanArrays &out) {
    for (int b = 0; b < p->B; b++) {
        if (only && !(*only)[b]) continue;
        if (take && p->h_cmd.p[b].flags != 0) {
            take->cand.push_back(b); take->sv.push_back(pl.sv[b]); take->newest.push_back(pl.newest[b]); take->bound.push_back(pl.bound[b]); take->f_last.push_back(pl.f_last[b]);
            continue;
        }
        std::memcpy(out.x + p->xoff[b], p->h_x.p + p->xoff[b], sizeof(double) * (p->xoff[b + 1] - p->xoff[b]));
        out.status[b] = pl.sv[b].status();
        if (out.iters) out.iters[b] = pl.sv[b].iterations();
        if (out.evals) out.evals[b] = pl.sv[b].evaluations();
        if (out.objective) out.objective[b] = pl.sv[b].value();
    }
}

// Device-vector optimisation: the host runs one SolverDV (scalars + decisions) per candidate, the device owns every
// vector.  A round = k_lbfgs_pre (history update + two-loop recursion for candidates that just accepted a step, then the
// trial point) -> k_forward -> k_penalty -> k_backward -> k_lbfgs_post; 32 B of commands go down and 40 B of results
// come back per candidate, through mapped host memory.
// `only` (optional, [B]): candidates with only[b] == 0 take no part - their x, status, counters and objective are left untouched
// (used to re-run, on this path, candidates that failed on the resident kernel).
// `take` (optional): see TakeOver; returns 2 when the candidates still running were handed over.  1: the caller falls back to host vectors.
static int optimize_device_vectors(frx_problem *p, const frx_lbfgs_params &pm, const frx::PlanSwitches &sw, const frx::PlanArrays &out,
                                   const std::vector<char> *only = nullptr, TakeOver *take = nullptr) {
    const int B = p->B, m = pm.mem_size;
    const frx::DvPreGeometry geom = frx::dv_pre_geometry(p->geo.maxXb, sw);
    if (geom.E == 0 || m > 512 || m < 1) return 1;
    const size_t HS = frx::dv_row_stride(p->geo.maxXb, geom.E, geom.W, sw.dv_tight);   // rows as long as the longest candidate's vector needs
    const int rc_buf = reserve_dv_buffers(p, m, HS);
    if (rc_buf != FRX_OK) return rc_buf;
    frx::DvLaunch dv;
    dv.xoff = p->d_xoff.p; dv.x = p->d_x.p; dv.g = p->d_g.p; dv.xp = p->d_xp.p; dv.gp = p->d_gp.p; dv.d = p->d_dir.p;
    dv.S = p->d_S.p; dv.Y = p->d_Y.p; dv.ys = p->d_ys.p; dv.gt = p->d_gt.p; dv.ld = (size_t)p->NX; dv.hs = HS; dv.m = m; dv.B = B; dv.E = geom.E; dv.W = geom.W; dv.PF = geom.PF; dv.BLK = geom.BLK;
    std::memcpy(p->h_x.p, out.x, sizeof(double) * p->NX);
    HIP_TRY(hipMemcpyAsync(p->d_x.p, p->h_x.p, sizeof(double) * p->NX, hipMemcpyHostToDevice, p->stream));
    HIP_TRY(hipMemsetAsync(p->d_ys.p, 0, sizeof(double) * (size_t)B * m, p->stream));
    HIP_TRY(hipMemsetAsync(p->d_gt.p, 0, sizeof(double) * (size_t)B * m * 4, p->stream));
    DvPlan pl(B);
    for (int b = 0; b < B; b++) {
        pl.sv[b].start(p->xoff[b + 1] - p->xoff[b], pm, p->h_cmd.p + b);
        if (only && !(*only)[b]) pl.sv[b].give_up(0);                          // not part of this run
    }
    const bool fused_post = p->geo.solver == frx::SOLVER_KNOT_PCR, mailbox = fused_post && sw.mailbox;
    TapGuard tap_guard{p};
    if (fused_post) { const int rc_tap = arm_tap(p, sw, mailbox, dv); if (rc_tap != FRX_OK) return rc_tap; }
    double t_dev = 0.0, t_host = 0.0;
    long rounds = 0;
    p->trace.clear();
    bool handed_over = false;
    const auto t0 = clk::now();
    for (;;) {
        bool any_eval = false;
        int running = 0;
        for (int b = 0; b < B; b++) { any_eval |= (p->h_cmd.p[b].flags & frx::DV_EVAL) != 0; running += p->h_cmd.p[b].flags != 0; }
        if (running == 0) break;
        if (take && take->capacity > 0 && running <= take->capacity && rounds >= take->not_before) { handed_over = true; break; }   // the rest continues on the resident kernel
        for (int b = 0; b < B; b++)
            if (p->h_cmd.p[b].flags & frx::DV_ADVANCE) { pl.newest[b] = p->h_cmd.p[b].slot; pl.bound[b] = p->h_cmd.p[b].bound; }  // the pair this round stores
        auto td = clk::now();
        HIP_TRY((hipError_t)frx::launch_lbfgs_pre(dv, p->h_cmd.p, p->h_res.p, p->stream));
        if (any_eval) {
            if (mailbox) p->tap.round++;
            // (fault injection, tests: FRX_DEBUG_DROP_ROUND=k leaves k_backward_knot out of round k, so that round's completion is never posted)
            if (rounds == sw.drop_round) HIP_TRY((hipError_t)frx::launch_eval(p, p->d_x.p, p->d_f.p, p->d_g.p, p->stream, false));
            else HIP_TRY((hipError_t)frx::launch_eval(p, p->d_x.p, p->d_f.p, p->d_g.p, p->stream, true));
            if (!fused_post) HIP_TRY((hipError_t)frx::launch_lbfgs_post(dv, p->d_f.p, p->h_cmd.p, p->h_res.p, p->stream));
        }
        const int rc_wait = wait_round(p, mailbox && any_eval, sw.round_timeout_ms);
        if (rc_wait != FRX_OK) return rc_wait;
        t_dev += ms_since(td);
        auto th = clk::now();
        feed_round(p, pl, sw.trace);
        t_host += ms_since(th);
        rounds++;
    }
    p->stats = {ms_since(t0), t_dev, t_host, (double)rounds};
    HIP_TRY(hipMemcpyAsync(p->h_x.p, p->d_x.p, sizeof(double) * p->NX, hipMemcpyDeviceToHost, p->stream));
    HIP_TRY(hipStreamSynchronize(p->stream));
    if (handed_over) take->spent = p->stats;
    collect_or_hand_over(p, pl, only, handed_over ? take : nullptr, out);
    return handed_over ? 2 : FRX_OK;
}

// ---- the resident round kernel's host side (frx_round_kernel.hpp): ONE launch per plan ----

// A resident launch needs ALL of its workgroups on the chip at once (one per CU: ~154 KB of LDS each).  Two launches that share a
// device - two shards of frx_multi on one GPU, two user threads - could each get a partially resident grid, and neither census would
// ever complete.  Launches of this process are therefore serialised per device: the second plan waits for the first one's kernel to
// leave (another PROCESS on the same device is caught by the census bound instead: 250 ms, then the per-stage path).
static std::mutex &resident_device_lock(int device) {
    static std::mutex table_lock;
    static std::map<int, std::unique_ptr<std::mutex>> table;
    std::lock_guard<std::mutex> g(table_lock);
    std::unique_ptr<std::mutex> &m = table[device];
    if (!m) m.reset(new std::mutex());
    return *m;
}

// the environment of THIS plan (read at every plan: tests and A/B runs change it between two plans of one process)
static frx::ResidentKnobs resident_knobs_from_env() {
    frx::ResidentKnobs kn;
    auto num = [](const char *name, int unset) { const char *e = std::getenv(name); return e ? std::atoi(e) : unset; };
    kn.e = num("FRX_RESIDENT_E", 0);
    kn.g = num("FRX_RESIDENT_G", 0);
    kn.clusters_set = std::getenv("FRX_RESIDENT_CLUSTERS") != nullptr; kn.clusters = num("FRX_RESIDENT_CLUSTERS", 0);
    kn.queue = std::getenv("FRX_RESIDENT_QUEUE") ? (frx::env_off("FRX_RESIDENT_QUEUE") ? 0 : 1) : -1;
    kn.queue_max = num("FRX_RESIDENT_QUEUE_MAX", 3);
    kn.host_threads_set = std::getenv("FRX_RESIDENT_HOST_THREADS") != nullptr; kn.host_threads = num("FRX_RESIDENT_HOST_THREADS", 0);
    kn.scan_pause = std::max(0, num("FRX_RESIDENT_SCAN_PAUSE", 0));
    kn.cmd_stride = num("FRX_RESIDENT_CMD_STRIDE", 4) == 1 ? 1 : 4;
    kn.fast_control = !frx::env_off("FRX_RESIDENT_FAST_CONTROL");
    kn.timed_read = frx::env_is("FRX_RESIDENT_TIMED_READ", '1');
    kn.early_read = !frx::env_off("FRX_RESIDENT_EARLY_READ");
    kn.write_through = frx::env_is("FRX_RESIDENT_WRITE_THROUGH", '1');   // no cluster trusts its XCD census: write-through stores everywhere (what a cluster spread over XCDs does)
    kn.speculate = std::max(0, std::min(2, num("FRX_RESIDENT_SPECULATE", 2)));
    kn.no_ll20 = std::getenv("FRX_RESIDENT_NO_LL20") != nullptr;
    kn.stamp_round = std::max(0, num("FRX_RESIDENT_STAMP_ROUND", 0));
    kn.timeout_ms = round_timeout_ms();
    kn.numa = !frx::env_off("FRX_NUMA");
    return kn;
}

// the diagnostics a plan was asked for, from their buffers before the launch to their read-back after it
struct RoundDiag {
    bool dbg = false; int log_cands = 0; size_t log_doubles = 0;    // direction log (frx_debug.h): [B] record counts, then dirlog_cands x dirlog_cap records {s, y, g, d, slot, pair count}
    bool prof = false, stamps = false;                               // FRX_RESIDENT_PROF: segment times; and (unless = 2: the stamps' stores perturb what they measure) candidate 0's phase stamps
    // FRX_RESIDENT_TRACE="lo,hi[,file]" (with FRX_RESIDENT_PROF): timeline of cluster 0 for the phases lo <= n < hi - every workgroup's thread 0 logs
    // (segment id, phase, 100 MHz wall clock) - written as text to `file` (default frx_round_trace.txt) after the plan (scripts/r04/round_timeline.py)
    DevBuf<unsigned long long> d_trace; unsigned trace_lo = 0, trace_hi = 0; std::string trace_file = "frx_round_trace.txt";
    static constexpr int trace_cap = 2048;
};

// exchange buffers and mailboxes of the plan's geometry; 1: they do not fit
static int ensure_round_buffers(frx_problem *p, const frx::ResidentPlan &pl) {
    const int B = p->B, S = pl.S, G = pl.G, NXP = pl.NXP;
    if (p->rk_B == B && p->rk_S == S && p->rk_G == G && p->rk_NXP == NXP) return FRX_OK;
    p->rk_B = 0;
    NumaScope numa_alloc(p->device);                                                  // the mailboxes' pages come from the device's NUMA node
    if (p->d_pubsyg.alloc((size_t)S * (3 * NXP + 2)) != hipSuccess || p->d_part.alloc((size_t)S * G * 512) != hipSuccess ||
        p->d_upub.alloc((size_t)S * 258) != hipSuccess || p->d_dpub.alloc((size_t)S * 2 * NXP) != hipSuccess ||
        p->d_out20ll.alloc((size_t)p->P * 40) != hipSuccess || p->d_rwords.alloc(pl.n_words) != hipSuccess || p->h_rcmd.alloc((size_t)8 * S) != hipSuccess || p->h_rres.alloc((size_t)8 * S) != hipSuccess ||
        p->d_xp.reserve(p->NX) != hipSuccess || p->d_gp.reserve(p->NX) != hipSuccess || p->d_dir.reserve(p->NX) != hipSuccess) {
        (void)hipGetLastError();
        return 1;
    }
    p->rk_B = B; p->rk_S = S; p->rk_G = G; p->rk_NXP = NXP;
    return FRX_OK;
}

// direction-log, profile and timeline buffers, zeroed on the plan's stream
static int prepare_round_diagnostics(frx_problem *p, const frx::ResidentPlan &pl, bool takeover, RoundDiag &dg) {
    const int B = p->B, S = pl.S, G = pl.G;
    dg.log_cands = std::min(p->dirlog_cands, B);
    dg.dbg = p->dirlog_cap > 0 && dg.log_cands > 0;
    dg.log_doubles = dg.dbg ? (size_t)B + (size_t)dg.log_cands * p->dirlog_cap * (4 * (size_t)pl.NXP + 2) : 0;
    p->dirlog.clear(); p->dirlog_nxp = pl.NXP;
    if (dg.dbg) {
        if (p->d_rdbg.reserve(dg.log_doubles) != hipSuccess) return fail(FRX_ERR_ALLOC, "direction log does not fit the device");
        HIP_TRY(hipMemsetAsync(p->d_rdbg.p, 0, sizeof(double) * dg.log_doubles, p->stream));
    }
    const char *prof_env = takeover ? nullptr : std::getenv("FRX_RESIDENT_PROF");
    dg.prof = prof_env != nullptr;
    dg.stamps = dg.prof && prof_env[0] != '2';
    p->rprof.clear();
    if (!dg.prof) return FRX_OK;
    if (p->d_rprof.reserve((size_t)S * (G + 1) * 16) != hipSuccess) return 1;
    HIP_TRY(hipMemsetAsync(p->d_rprof.p, 0, sizeof(unsigned long long) * (size_t)S * (G + 1) * 16, p->stream));
    if (const char *tr_env = std::getenv("FRX_RESIDENT_TRACE")) {
        unsigned lo = 0, hi = 0; char fbuf[512] = {0};
        const int nf = std::sscanf(tr_env, "%u,%u,%511s", &lo, &hi, fbuf);
        if (nf >= 2 && hi > lo && dg.d_trace.alloc((size_t)G * dg.trace_cap) == hipSuccess) {
            HIP_TRY(hipMemsetAsync(dg.d_trace.p, 0, sizeof(unsigned long long) * (size_t)G * dg.trace_cap, p->stream));
            dg.trace_lo = lo; dg.trace_hi = hi;
            if (nf == 3) dg.trace_file = fbuf;
        }
    }
    if (!dg.stamps && p->d_stamps.p) HIP_TRY(hipMemsetAsync(p->d_stamps.p, 0, 64 * sizeof(long long), p->stream));
    if (dg.stamps) {                                                                  // phase stamps of candidate 0's forward / adjoint bodies (last evaluation)
        if (!p->d_stamps.p) HIP_TRY(p->d_stamps.alloc(FRX_STAMP_SLOTS));
        HIP_TRY(hipMemsetAsync(p->d_stamps.p, 0, 64 * sizeof(long long), p->stream));
    }
    return FRX_OK;
}

// state of this launch: all polled words zero, mailboxes empty
static int zero_round_state(frx_problem *p, const frx::ResidentPlan &pl) {
    const int S = pl.S, NXP = pl.NXP;
    HIP_TRY(hipMemsetAsync(p->d_rwords.p, 0, sizeof(unsigned) * pl.n_words, p->stream));
    HIP_TRY(hipMemsetAsync(p->d_out20ll.p, 0, sizeof(double) * (size_t)p->P * 40, p->stream));
    HIP_TRY(hipMemsetAsync(p->d_dpub.p, 0, sizeof(double) * (size_t)S * 2 * NXP, p->stream));           // granules of the cluster's hand-offs: tag 0 = nothing yet
    HIP_TRY(hipMemsetAsync(p->d_pubsyg.p, 0, sizeof(double) * (size_t)S * (3 * NXP + 2), p->stream));   // the point and gradient the cluster reads: zero beyond n (padding of s and y)
    std::memset(p->h_rcmd.p, 0, sizeof(unsigned long long) * 8 * S);
    std::memset(p->h_rres.p, 0, sizeof(unsigned long long) * 8 * S);
    return FRX_OK;
}

// The dense state of every straggler from its history rows: read back (1.5 MB per candidate), R = S^T Y (triangular part), its inverse, Y^T Y and D on the
// set-up pool's threads (frx_compact.hpp: 2 x 128 x 128 dot products of length n per candidate), uploaded as the clusters' take-over arrays.  1: they do not fit
static int upload_takeover_state(frx_problem *p, int S, int m, const TakeOver &take, frx::RoundLaunch &rl) {
    const size_t HS = p->dv_hs, rowblk = (size_t)m * HS;
    std::vector<double> hS((size_t)S * rowblk), hY((size_t)S * rowblk), rinv((size_t)S * 128 * 129), yy((size_t)S * 128 * 128), vd((size_t)S * 128);
    for (int k = 0; k < S; k++) {
        const int b = take.cand[k];
        HIP_TRY(hipMemcpyAsync(hS.data() + (size_t)k * rowblk, p->d_S.p + (size_t)b * rowblk, sizeof(double) * rowblk, hipMemcpyDeviceToHost, p->stream));
        HIP_TRY(hipMemcpyAsync(hY.data() + (size_t)k * rowblk, p->d_Y.p + (size_t)b * rowblk, sizeof(double) * rowblk, hipMemcpyDeviceToHost, p->stream));
    }
    HIP_TRY(hipStreamSynchronize(p->stream));
    frx::TaskPool::get().run(S, frx::setup_threads(S, 8000.0), [&](int k, int) {
        const int b = take.cand[k];
        frx::compact_from_history(m, p->xoff[b + 1] - p->xoff[b], HS, take.bound[k], take.newest[k], hS.data() + (size_t)k * rowblk, hY.data() + (size_t)k * rowblk, 129,
                                  rinv.data() + (size_t)k * 128 * 129, yy.data() + (size_t)k * 128 * 128, vd.data() + (size_t)k * 128);
    });
    std::vector<int> ints((size_t)3 * S);
    for (int k = 0; k < S; k++) { ints[k] = take.cand[k]; ints[S + k] = take.newest[k]; ints[2 * S + k] = take.bound[k]; }
    if (p->d_rs_int.reserve(ints.size()) != hipSuccess || p->d_rs_f.reserve((size_t)S) != hipSuccess || p->d_rs_rinv.reserve(rinv.size()) != hipSuccess ||
        p->d_rs_yy.reserve(yy.size()) != hipSuccess || p->d_rs_vd.reserve(vd.size()) != hipSuccess) { (void)hipGetLastError(); return 1; }
    HIP_TRY(hipMemcpy(p->d_rs_int.p, ints.data(), sizeof(int) * ints.size(), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(p->d_rs_f.p, take.f_last.data(), sizeof(double) * S, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(p->d_rs_rinv.p, rinv.data(), sizeof(double) * rinv.size(), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(p->d_rs_yy.p, yy.data(), sizeof(double) * yy.size(), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(p->d_rs_vd.p, vd.data(), sizeof(double) * vd.size(), hipMemcpyHostToDevice));
    rl.rs_cand = p->d_rs_int.p; rl.rs_newest = p->d_rs_int.p + S; rl.rs_bound = p->d_rs_int.p + 2 * S;
    rl.rs_f = p->d_rs_f.p; rl.rs_S = p->d_S.p; rl.rs_Y = p->d_Y.p; rl.rs_hs = HS; rl.rs_rinv = p->d_rs_rinv.p; rl.rs_yy = p->d_rs_yy.p; rl.rs_vd = p->d_rs_vd.p;
    return FRX_OK;
}

// everything else the launch takes: the handle's buffers, the plan's geometry, the knobs, the line-search parameters the leader predicts with
static void round_launch_args(const frx::ResidentKnobs &kn, const frx_lbfgs_params &pm, frx_problem *p, const frx::ResidentPlan &pl, const RoundDiag &dg, frx::RoundLaunch &rl) {
    rl.x = p->d_x.p; rl.g = p->d_g.p; rl.xp = p->d_xp.p; rl.gp = p->d_gp.p; rl.d = p->d_dir.p; rl.f = p->d_f.p; rl.T = p->d_T.p; rl.C = p->d_C.p; rl.out20 = p->d_out20.p;
    rl.pubsyg = p->d_pubsyg.p; rl.part = p->d_part.p; rl.upub = p->d_upub.p; rl.dpub = p->d_dpub.p;
    rl.out20ll = kn.no_ll20 ? nullptr : (unsigned long long *)p->d_out20ll.p;
    rl.dbg = dg.dbg ? p->d_rdbg.p : nullptr; rl.dbg_cap = dg.dbg ? p->dirlog_cap : 0; rl.dbg_cands = dg.dbg ? dg.log_cands : 0;
    rl.words = p->d_rwords.p; rl.h_cmd = p->h_rcmd.p; rl.h_res = p->h_rres.p;
    if (!p->d_rargs.p && p->d_rargs.alloc(frx::round_args_bytes()) != hipSuccess) { (void)hipGetLastError(); p->d_rargs.p = nullptr; }
    rl.args_dev = p->d_rargs.p;
    rl.timeout_ticks = (unsigned long long)(kn.timeout_ms * 1e5);                     // wall_clock64: 100 MHz
    rl.B = p->B; rl.S = pl.S; rl.G = pl.G; rl.m = pm.mem_size; rl.E = pl.E; rl.NXP = pl.NXP;
    rl.prof = dg.prof ? p->d_rprof.p : nullptr;
    if (dg.d_trace.p) { rl.trace = dg.d_trace.p; rl.trace_cap = dg.trace_cap; rl.trace_lo = dg.trace_lo; rl.trace_hi = dg.trace_hi; }
    rl.fast_control = (kn.fast_control ? 1 : 0) | (kn.timed_read ? 2 : 0) | (kn.early_read ? 0 : 4) | (kn.write_through ? 8 : 0);
    rl.stamp_round = dg.prof ? kn.stamp_round : 0;
    rl.cmd_stride = kn.cmd_stride;                                                    // 4: one cache line per cluster
    rl.ls_ftol = pm.f_dec_coeff; rl.ls_gtol = pm.s_curv_coeff; rl.ls_min_step = pm.min_step; rl.ls_max_step = pm.max_step; rl.ls_xtol = pm.xtol; rl.ls_max_linesearch = pm.max_linesearch;
    // What the leader expects of the host (frx_round_kernel.hpp): 0 nothing, it waits for every command; 1 the acceptance of a trial (ADVANCE, next
    // slot, step 1: lbfgs.hpp:1418); 2 also the next trial step of a running search (default).  Every expectation is checked against the host's
    // command word before the next result is posted.  Measured, production kernel, us per round: 32 candidates 31.5 (round 2's rule: first-trial
    // acceptances only) -> 30.7 (level 2); one candidate 30.3 -> 29.9.  FRX_RESIDENT_SPECULATE=0|1|2 overrides.
    rl.speculate = (pm.min_step <= 1.0 && 1.0 <= pm.max_step) ? kn.speculate : 0;   // the predicted ADVANCE carries step 1 (lbfgs.hpp:1418)
}

// what the launch left behind: status word (*device_status), prediction counters, and whatever diagnostics the plan was asked for
static int read_back_diagnostics(frx_problem *p, const frx::ResidentPlan &pl, const RoundDiag &dg, unsigned *device_status) {
    const int B = p->B, S = pl.S, G = pl.G;
    const unsigned *tail = p->d_rwords.p + (size_t)frx::ROUND_WORDS_PER_CAND * S;    // census, status, [S][G] XCC ids, [B][4] prediction counters
    unsigned st[2] = {0, 0};
    HIP_TRY(hipMemcpy(st, tail, sizeof(st), hipMemcpyDeviceToHost));
    p->resident_status = *device_status = st[1];
    {
        std::vector<unsigned> sc(4 * (size_t)B, 0u);
        HIP_TRY(hipMemcpy(sc.data(), tail + 2 + (size_t)S * G, sizeof(unsigned) * sc.size(), hipMemcpyDeviceToHost));
        for (int q = 0; q < 4; q++) { p->spec_counts[q] = 0; for (int b = 0; b < B; b++) p->spec_counts[q] += sc[4 * (size_t)b + q]; }
    }
    if (std::getenv("FRX_RESIDENT_HOST_STATS")) {                                     // diagnostic: where the workgroups of every cluster ran (XCC id of each)
        std::vector<unsigned> xc((size_t)S * G, 0u);
        HIP_TRY(hipMemcpy(xc.data(), tail + 2, sizeof(unsigned) * xc.size(), hipMemcpyDeviceToHost));
        int one_xcd = 0;
        std::string line;
        for (int k = 0; k < S; k++) {
            bool same = true;
            for (int w = 1; w < G; w++) same = same && (xc[(size_t)k * G + w] & 0xFFu) == (xc[(size_t)k * G] & 0xFFu);
            one_xcd += same ? 1 : 0;
            line += " [";
            for (int w = 0; w < G; w++) {                                // XCD : shader engine . shader array . CU of every workgroup (leader first, dense last)
                const unsigned e = xc[(size_t)k * G + w];
                line += std::to_string((int)(e & 0xFFu) - 1) + ":" + std::to_string((e >> 13) & 7u) + "." + std::to_string((e >> 12) & 1u) + "." + std::to_string((e >> 8) & 15u) + (w + 1 < G ? " " : "");
            }
            line += "]";
        }
        std::fprintf(stderr, "[frx] clusters on one XCD: %d of %d;%s\n", one_xcd, S, line.c_str());
    }
    if (dg.dbg) {
        p->dirlog.resize(dg.log_doubles);
        HIP_TRY(hipMemcpy(p->dirlog.data(), p->d_rdbg.p, sizeof(double) * dg.log_doubles, hipMemcpyDeviceToHost));
    }
    return FRX_OK;
}

// ... and of a plan that succeeded: the timeline file and the segment profile (the last 32 words: the bodies' cycle stamps)
static int read_back_profile(frx_problem *p, const frx::ResidentPlan &pl, const RoundDiag &dg, int stamp_round) {
    const int S = pl.S, G = pl.G;
    if (dg.d_trace.p) {
        std::vector<unsigned long long> tr((size_t)G * dg.trace_cap);
        HIP_TRY(hipMemcpy(tr.data(), dg.d_trace.p, sizeof(unsigned long long) * tr.size(), hipMemcpyDeviceToHost));
        if (FILE *f = std::fopen(dg.trace_file.c_str(), "w")) {
            std::fprintf(f, "# workgroup segment phase ticks(100MHz, 40 bits)   G=%d\n", G);
            for (int w = 0; w < G; w++)
                for (int i = 0; i < dg.trace_cap; i++) {
                    const unsigned long long e = tr[(size_t)w * dg.trace_cap + i];
                    if (!e) break;
                    std::fprintf(f, "%d %llu %llu %llu\n", w, e >> 56, (e >> 40) & 0xFFFFull, e & 0xFFFFFFFFFFull);
                }
            std::fclose(f);
        }
    }
    if (dg.prof) {
        p->rprof.resize((size_t)S * (G + 1) * 16 + 32);                                // [S][G][16] segment sums, [S][16] host-wait histogram; the last 32 words: the bodies' cycle stamps
        HIP_TRY(hipMemcpy(p->rprof.data(), p->d_rprof.p, sizeof(unsigned long long) * (size_t)S * (G + 1) * 16, hipMemcpyDeviceToHost));
        if (!p->d_stamps.p) { HIP_TRY(p->d_stamps.alloc(FRX_STAMP_SLOTS)); HIP_TRY(hipMemset(p->d_stamps.p, 0, 64 * sizeof(long long))); }
        HIP_TRY(hipMemcpy(p->rprof.data() + (size_t)S * (G + 1) * 16, p->d_stamps.p + (stamp_round > 0 ? 32 : 0), 32 * sizeof(long long), hipMemcpyDeviceToHost));   // the last evaluation's stamps, or those of evaluation FRX_RESIDENT_STAMP_ROUND
    }
    return FRX_OK;
}

// Resident optimisation: the host runs the same SolverDV state machines as optimize_device_vectors, but talks to each candidate's cluster through its
// own mailbox and never waits for the batch: a candidate's next command is posted the moment its result arrives.  Returns FRX_OK, a negative
// frx_status, or 1 = not applicable / the device gave up (resident_status says why): the caller then runs the one-launch-per-stage path from the untouched x.
// `take` (optional): not a plan from its start but the continuation of the candidates a per-stage batch handed over (TakeOver above): cluster k runs candidate
// take->cand[k] from its pending command on, with the per-stage path's vectors and a dense state rebuilt from its history (frx_compact.hpp); everybody
// else's results are left alone.
static int optimize_resident(frx_problem *p, const frx_lbfgs_params &pm, double *x, int *status, int *iters, int *evals, double *objective, TakeOver *take = nullptr) {
    const int B = p->B, m = pm.mem_size;
    const int Bsel = take ? (int)take->cand.size() : B;                              // candidates that run here
    p->resident_used = 0; p->resident_status = 0; p->resident_failed = 0;
    const frx::ResidentKnobs kn = resident_knobs_from_env();
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, p->device) != hipSuccess) return 1;
    int min_n = INT_MAX;
    for (int q = 0; q < Bsel; q++) { const int b = take ? take->cand[q] : q; min_n = std::min(min_n, p->xoff[b + 1] - p->xoff[b]); }
    const frx::ResidentPlan pl = frx::resident_plan({p->geo.solver, p->geo.knot_threads, m, B, Bsel, min_n, p->geo.maxXb, p->geo.maxN, p->geo.ppw, prop.multiProcessorCount,
                                                     p->resident_mode, take != nullptr, p->dv_mem, p->d_S.p != nullptr}, kn);
    if (!pl.applicable) return 1;
    const int S = pl.S, G = pl.G;
    const size_t lds = frx::round_lds_bytes(p->geo, m, pl.E);
    if (lds == 0 || lds > 160 * 1024) return 1;
    int rc = ensure_round_buffers(p, pl);
    if (rc != FRX_OK) return rc;
    RoundDiag dg;
    if ((rc = prepare_round_diagnostics(p, pl, take != nullptr, dg)) != FRX_OK) return rc;
    if ((rc = zero_round_state(p, pl)) != FRX_OK) return rc;
    frx::RoundLaunch rl;
    if (!take) {
        std::memcpy(p->h_x.p, x, sizeof(double) * p->NX);
        HIP_TRY(hipMemcpyAsync(p->d_x.p, p->h_x.p, sizeof(double) * p->NX, hipMemcpyHostToDevice, p->stream));
    } else if ((rc = upload_takeover_state(p, S, m, *take, rl)) != FRX_OK) return rc;
    round_launch_args(kn, pm, p, pl, dg, rl);
    struct StampGuard { frx_problem *q; ~StampGuard() { q->dp.stamps = nullptr; } } stamp_guard{p};
    if (dg.stamps) p->dp.stamps = p->d_stamps.p;

    const bool tracing = std::getenv("FRX_TRACE") != nullptr;
    if (!take) p->trace.clear();                                                      // (a take-over continues the per-stage part's trace)
    frx::ResidentMailbox mb(S, B, p->xoff.data(), pm, p->h_rcmd.p, p->h_rres.p, rl.cmd_stride, {status, iters, evals, objective, tracing ? &p->trace : nullptr});
    if (!take) {
        for (int b = 0; b < B; b++) status[b] = 0;
        mb.start();
    } else mb.start_takeover(take->cand, take->sv);
    // the threads that talk to the device stay on the device's NUMA node for the length of the plan (FRX_NUMA=0: wherever the scheduler puts them);
    // the caller's own affinity is put back when the plan is over.  Looked up (cached per device) before the launch: the clusters spin from then on
    cpu_set_t numa_set, caller_set;
    const bool numa_pin = kn.numa && frx::device_numa_cpus(p->device, &numa_set);
    std::unique_lock<std::mutex> device_slot(resident_device_lock(p->device));        // one resident grid per device at a time (see above)
    const auto t0 = clk::now();
    HIP_TRY((hipError_t)frx::launch_round(p->dp, p->geo, rl, p->stream));
    mb.post_first();
    // Sixteen clusters per service thread, at most four threads (round 4; four per thread, at most eight, until then): 1, 2, 4 and 8 threads measure the same round
    // (25.2-25.4 us at 32 clusters, profiles/r04_host_threads.txt) - a scan of 16 mailboxes and the line-search step of those that answered take a few
    // microseconds of a 25 us round - and every one of them SPINS for the length of the plan: under a CPU quota (the GPU boxes of this project run the
    // process with 16 CPUs' worth) eight ranks of a node with nine spinning threads each are throttled to a crawl, eight ranks with two are not.
    // ... and no more of them than this plan's share of the CPUs the process may use: cgroup quota and affinity mask, divided by
    // the plans that spin next to this one - the other ranks of the node (LOCAL_WORLD_SIZE, set by torch.distributed.run; FRX_LOCAL_RANKS overrides)
    // and the other shards of a frx_multi job in this process - minus one CPU for the rank's main (interpreter) thread.  Eight ranks under the GPU
    // boxes' quota of 16 CPUs: the caller alone serves the mailboxes (one thread measures the same round as eight, profiles/r04_host_threads.txt).
    int nsrv = frx::mailbox_threads(S);
    if (kn.host_threads_set) nsrv = std::max(1, std::min(kn.host_threads, S));
    std::vector<frx::ResidentMailbox::ServeStats> served(nsrv);
    const bool caller_saved = numa_pin && pthread_getaffinity_np(pthread_self(), sizeof(caller_set), &caller_set) == 0;
    if (caller_saved) (void)pthread_setaffinity_np(pthread_self(), sizeof(numa_set), &numa_set);
    auto serve = [&](int tid) {
        if (numa_pin && tid > 0) (void)pthread_setaffinity_np(pthread_self(), sizeof(numa_set), &numa_set);
        served[tid] = mb.serve(tid, nsrv, kn.timeout_ms, kn.scan_pause, [p] { return hipStreamQuery(p->stream) != hipErrorNotReady; });
    };
    {
        std::vector<std::thread> helpers;
        for (int tid = 1; tid < nsrv; tid++) helpers.emplace_back(serve, tid);
        serve(0);
        for (auto &h : helpers) h.join();
    }
    if (caller_saved) (void)pthread_setaffinity_np(pthread_self(), sizeof(caller_set), &caller_set);
    if (std::getenv("FRX_RESIDENT_HOST_STATS")) {                                     // diagnostic: how often a service thread looks at each of its mailboxes
        const double wall_us = 1e3 * ms_since(t0);
        for (int tid = 0; tid < nsrv; tid++) std::fprintf(stderr, "[frx] mailbox thread %d: %ld scans of %d mailboxes in %.0f us = %.3f us per scan, busy %.1f ms\n", tid, served[tid].scans, (int)((long)S * (tid + 1) / nsrv) - (int)((long)S * tid / nsrv), wall_us, wall_us / std::max(1L, served[tid].scans), served[tid].busy_ms);
    }
    rc = FRX_OK;
    double t_host = 0.0;
    for (const auto &s : served) t_host = std::max(t_host, s.busy_ms);
    if (mb.abort_code() == 1) rc = 1;
    else if (mb.abort_code() == 2) rc = fail(FRX_ERR_TIMEOUT, "resident round kernel: no result within FRX_ROUND_TIMEOUT_MS");
    mb.quit_all();
    const int wrc = wait_stream(p->stream, 3.0 * kn.timeout_ms + 1000.0, "resident round kernel");   // bounded drain: the kernel's own spins expire after the same timeout
    if (wrc != FRX_OK) return wrc;
    device_slot.unlock();                                                             // the kernel has left the chip
    unsigned device_status = 0;
    const int rc_diag = read_back_diagnostics(p, pl, dg, &device_status);
    if (rc_diag != FRX_OK) return rc_diag;
    if (rc < 0) return rc;
    if (rc != FRX_OK || device_status != 0) return 1;
    const long rounds = mb.busiest();
    const double ms = ms_since(t0);
    p->stats = {ms, ms - t_host, t_host, (double)rounds};
    if (!take) HIP_TRY(hipMemcpy(x, p->d_x.p, sizeof(double) * p->NX, hipMemcpyDeviceToHost));
    else                                                                              //  a take-over's result: the stragglers' points only - everybody else's x is final already
        for (int b : take->cand) HIP_TRY(hipMemcpy(x + p->xoff[b], p->d_x.p + p->xoff[b], sizeof(double) * (size_t)(p->xoff[b + 1] - p->xoff[b]), hipMemcpyDeviceToHost));
    if ((rc = read_back_profile(p, pl, dg, rl.stamp_round)) != FRX_OK) return rc;
    for (int q = 0; q < Bsel; q++) {                                                  // (a take-over counts its own candidates, not the per-stage part's failures)
        const int b = take ? take->cand[q] : q;
        if (status[b] < 0 && status[b] != frx::LBERR_MAXIMUMITERATION) p->resident_failed++;
    }
    p->resident_used = G; p->resident_clusters = S;
    return FRX_OK;
}

// final generate (CPU.hpp:1258-1263) and the reference's return value (CPU.hpp:1267)
static int finish_optimize(frx_problem *p, const double *x, double *C, double *T, double *jerk_cost) {
    int rc;
    std::vector<double> Tt(p->P), Cc((size_t)p->P * 18);
    rc = frx_forward(p, x, Tt.data(), Cc.data());
    if (rc != FRX_OK) return rc;
    if (T) std::copy(Tt.begin(), Tt.end(), T);
    if (C) std::copy(Cc.begin(), Cc.end(), C);
    if (jerk_cost) {
        for (int b = 0; b < p->B; b++) {
            double obj = 0.0;                                            // getTrajJerkCost, CPU.hpp:507-520
            for (int gp = p->poff[b]; gp < p->poff[b + 1]; gp++) {
                const double *c3 = &Cc[18 * (size_t)gp + 9], *c4 = c3 + 3, *c5 = c3 + 6;
                const double t1 = Tt[gp], t2 = t1 * t1, t3 = t2 * t1, t4 = t2 * t2, t5 = t4 * t1;
                obj += 36.0 * frx::dot3(c3, c3) * t1 + 144.0 * frx::dot3(c4, c3) * t2 + 192.0 * frx::dot3(c4, c4) * t3 +
                       240.0 * frx::dot3(c5, c3) * t3 + 720.0 * frx::dot3(c5, c4) * t4 + 720.0 * frx::dot3(c5, c5) * t5;
            }
            jerk_cost[b] = obj;
        }
    }
    return FRX_OK;
}


static int eval_failed(hipError_t e) { return fail(FRX_ERR_HIP, std::string("device evaluation failed: ") + hipGetErrorString(e)); }

// One evaluation of the whole batch for the host-vector plan: h_x -> h_f, h_g.  Zero-copy round trip: the kernels read x from and write (f, grad) to mapped,
// coherent host memory over PCIe (205 KB each way at the headline size), so a round is three launches and one completion poll - no hipMemcpyAsync calls
// (each costs more host time than the kernels it feeds).  FRX_ZERO_COPY=0 restores copies.
static int eval_host_vectors(frx_problem *p, bool zero_copy, double timeout_ms) {
    hipError_t e;
    // an expired wait of the one-launch form must not end the plan as a silent LBFGSERR_ROUNDING (NaN objectives): the evaluation is repeated
    // once with the stage kernels, which the handle keeps from then on (eval_cluster_status retires the form)
    for (int attempt = 0; attempt < 2; attempt++) {
        const bool fused = p->eval_fused != 0;
        if (zero_copy) {
            if ((e = (hipError_t)frx::launch_eval(p, p->h_x.p, p->h_f.p, p->h_g.p, p->stream, true)) != hipSuccess) return eval_failed(e);
            const int wrc = wait_stream(p->stream, timeout_ms, "device evaluation");
            if (wrc != FRX_OK) return wrc;
        } else {
            if ((e = hipMemcpyAsync(p->d_x.p, p->h_x.p, sizeof(double) * p->NX, hipMemcpyHostToDevice, p->stream)) != hipSuccess) return eval_failed(e);
            if ((e = (hipError_t)frx::launch_eval(p, p->d_x.p, p->d_f.p, p->d_g.p, p->stream, true)) != hipSuccess) return eval_failed(e);
            if ((e = hipMemcpyAsync(p->h_f.p, p->d_f.p, sizeof(double) * p->B, hipMemcpyDeviceToHost, p->stream)) != hipSuccess) return eval_failed(e);
            if ((e = hipMemcpyAsync(p->h_g.p, p->d_g.p, sizeof(double) * p->NX, hipMemcpyDeviceToHost, p->stream)) != hipSuccess) return eval_failed(e);
            if ((e = hipStreamSynchronize(p->stream)) != hipSuccess) return eval_failed(e);
        }
        if (!fused || frx::eval_cluster_status(p, p->h_f.p) == FRX_OK) return FRX_OK;
    }
    return FRX_OK;
}

// the host-vector plan: every vector on the host, the device evaluates (FRX_LBFGS=host, or nothing else could run)
static int optimize_host_vectors(frx_problem *p, const frx_lbfgs_params &pm, const frx::PlanSwitches &sw, const frx::PlanArrays &out) {
    std::memcpy(p->h_x.p, out.x, sizeof(double) * p->NX);
    int nt = std::max(1u, std::min<unsigned>(std::thread::hardware_concurrency(), (unsigned)p->B));
    if (sw.host_threads_set) nt = std::max(1, std::min(sw.host_threads, p->B));
    const int rc = drive_batch(p->B, p->xoff.data(), p->h_x.p, p->h_g.p, p->h_f.p, pm, nt, out.status, out.iters, out.evals, out.objective, &p->stats,
                               [&](int, const int *) { return eval_host_vectors(p, sw.zero_copy, sw.round_timeout_ms); });
    if (rc == FRX_OK) std::memcpy(out.x, p->h_x.p, sizeof(double) * p->NX);
    return rc;
}

// the two device-vector drivers as the route calls them (frx_plan_route.hpp)
struct DevicePaths {
    frx_problem *p; const frx_lbfgs_params &pm; const frx::PlanSwitches &sw; const frx::PlanArrays &out;
    int resident(TakeOver *take) { return optimize_resident(p, pm, out.x, out.status, out.iters, out.evals, out.objective, take); }
    int per_stage(const std::vector<char> *only, TakeOver *take) { return optimize_device_vectors(p, pm, sw, out, only, take); }
    unsigned device_status() const { return p->resident_status; }
    int capacity() const { hipDeviceProp_t prop; return hipGetDeviceProperties(&prop, p->device) == hipSuccess ? frx::resident_capacity(p->geo.maxXb, prop.multiProcessorCount) : -1; }
    int fail(int code, const char *text) { return ::fail(code, text); }
};


extern "C" {

int frx_optimize(frx_problem *p, const frx_lbfgs_params *params, double *x, double *C, double *T, double *jerk_cost,
                 double *objective, int *status, int *iters, int *evals) {
    if (!p || !params || !x || !status) return fail(FRX_ERR_INVALID_ARG, "null argument");
    if (p->penalty_only) return fail(FRX_ERR_INVALID_ARG, "this handle serves frx_penalty_eval[_device] only (frx_penalty_problem_create)");
    HIP_TRY(hipSetDevice(p->device));
    const frx::PlanSwitches sw = plan_switches_from_env();
    const frx::PlanArrays out{x, status, iters, evals, objective};
    DevicePaths paths{p, *params, sw, out};
    int rc = frx::plan_route({sw, p->lbfgs_mode, p->resident_mode, p->resident_retry, p->takeover_at, p->geo.solver, p->geo.knot_threads, params->mem_size, p->B, p->NX, p->xoff.data()}, out,
                             {p->resident_used, p->resident_retried, p->resident_failed, p->resident_clusters, p->taken_over, p->spec_counts}, p->stats, paths);
    if (rc > 0) rc = optimize_host_vectors(p, *params, sw, out);
    return rc != FRX_OK ? rc : finish_optimize(p, x, C, T, jerk_cost);
}

int frx_problem_set_resident(frx_problem *p, int enable) {
    if (!p) return fail(FRX_ERR_INVALID_ARG, "null argument");
    p->resident_mode = enable == 0 ? 0 : enable == 2 ? 2 : 1;
    return FRX_OK;
}
int frx_optimize_path(const frx_problem *p, int *resident_used, unsigned *device_status) {
    if (!p) return fail(FRX_ERR_INVALID_ARG, "null argument");
    if (resident_used) *resident_used = p->resident_used;
    if (device_status) *device_status = p->resident_status;
    return FRX_OK;
}
int frx_resident_profile(const frx_problem *p, unsigned long long *out, int cap_words) {
    if (!p) return fail(FRX_ERR_INVALID_ARG, "null argument");
    const int n = (int)p->rprof.size();
    if (out) std::memcpy(out, p->rprof.data(), sizeof(unsigned long long) * (size_t)std::min(n, std::max(cap_words, 0)));
    return n;
}
int frx_debug_direction_log(frx_problem *p, int cap_steps, int n_cands) {
    if (!p || cap_steps < 0 || n_cands < 0) return fail(FRX_ERR_INVALID_ARG, "null handle or negative size");
    p->dirlog_cap = cap_steps; p->dirlog_cands = cap_steps > 0 ? n_cands : 0;
    p->dirlog.clear();
    return FRX_OK;
}
int frx_debug_direction_log_read(const frx_problem *p, int cand, double *out, int cap_rows, int *rows, int *row_doubles) {
    if (!p || cand < 0) return fail(FRX_ERR_INVALID_ARG, "null handle or negative candidate");
    const size_t rec = 4 * (size_t)p->dirlog_nxp + 2;
    int n = 0;
    if (!p->dirlog.empty() && cand < std::min(p->dirlog_cands, p->B)) n = std::min((int)p->dirlog[cand], p->dirlog_cap);
    if (rows) *rows = n;
    if (row_doubles) *row_doubles = (int)rec;
    if (out && n > 0) std::memcpy(out, p->dirlog.data() + p->B + (size_t)cand * p->dirlog_cap * rec, sizeof(double) * rec * (size_t)std::min(n, std::max(cap_rows, 0)));
    return FRX_OK;
}
int frx_debug_set_resident_retry(frx_problem *p, int enable) {
    if (!p) return fail(FRX_ERR_INVALID_ARG, "null argument");
    p->resident_retry = enable ? 1 : 0;
    return FRX_OK;
}
int frx_debug_resident_predictions(const frx_problem *p, unsigned long long *out3) {
    if (!p || !out3) return fail(FRX_ERR_INVALID_ARG, "null argument");
    for (int q = 0; q < 3; q++) out3[q] = p->spec_counts[q];
    return FRX_OK;
}
int frx_debug_resident_clusters(const frx_problem *p, int *clusters) {
    if (!p || !clusters) return fail(FRX_ERR_INVALID_ARG, "null argument");
    *clusters = p->resident_clusters;
    return FRX_OK;
}
int frx_debug_resident_counts(const frx_problem *p, int *failed, int *retried) {
    if (!p) return fail(FRX_ERR_INVALID_ARG, "null argument");
    if (failed) *failed = p->resident_failed;
    if (retried) *retried = p->resident_retried;
    return FRX_OK;
}
int frx_debug_trace(const frx_problem *p, double *out, int cap_rows) {
    if (!p) return fail(FRX_ERR_INVALID_ARG, "null argument");
    const int rows = (int)(p->trace.size() / 7);
    if (out) std::memcpy(out, p->trace.data(), sizeof(double) * 7 * (size_t)std::min(rows, std::max(cap_rows, 0)));
    return rows;
}
int frx_debug_set_takeover_at(frx_problem *p, long rounds) {
    if (!p) return fail(FRX_ERR_INVALID_ARG, "null argument");
    p->takeover_at = rounds > 0 ? rounds : 0;
    return FRX_OK;
}
int frx_debug_taken_over(const frx_problem *p, int *candidates) {
    if (!p || !candidates) return fail(FRX_ERR_INVALID_ARG, "null argument");
    *candidates = p->taken_over;
    return FRX_OK;
}

int frx_optimize_stats(const frx_problem *p, double *out4) {
    if (!p || !out4) return fail(FRX_ERR_INVALID_ARG, "null argument");
    out4[0] = p->stats.ms; out4[1] = p->stats.ms_dev; out4[2] = p->stats.ms_host; out4[3] = p->stats.rounds;
    return FRX_OK;
}

int frx_lbfgs_minimize_batch(int count, const int *x_off, double *x, double *f_out, int *status, int *iters, int *evals,
                             const frx_lbfgs_params *params, frx_batch_eval_fn eval, void *instance, int n_threads) {
    if (count <= 0 || !x_off || !x || !params || !eval || !status) return fail(FRX_ERR_INVALID_ARG, "null argument or count <= 0");
    const int NX = x_off[count];
    std::vector<double> g(NX, 0.0), f(count, 0.0);
    auto eval_all = [&](int na, const int *ids) -> int {
        eval(instance, na, ids, x, f.data(), g.data());
        return FRX_OK;
    };
    return drive_batch(count, x_off, x, g.data(), f.data(), *params, std::max(1, n_threads), status, iters, evals, f_out, nullptr,
                       eval_all);
}

} // extern "C"
