// Which driver a plan takes and what happens when one gives up (frx_optimize): the resident round kernel first, a second chance on the per-stage rounds for
// candidates it failed on, per-stage rounds that hand their stragglers over to the resident kernel, a re-plan when that is refused, host vectors when nothing
// else runs.  Plain C++: no HIP and no getenv.  frx_optimize.cpp fills PlanSwitches from the environment once per call and plays the two drivers through a
// Paths object; tests/test_plan_route_cpu.py and tests/hostcheck/plan_route_main.cpp play them from a script.
#pragma once
#include <algorithm>
#include <climits>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/frx.h"
#include "frx_device.hpp"
#include "frx_lbfgs.hpp"

namespace frx {

// The environment of one frx_optimize call (plan_switches_from_env, frx_optimize.cpp); the defaults are the unset variables.
struct PlanSwitches {
    bool lbfgs_host = false;                    // FRX_LBFGS=h...: every vector on the host (bit-identical to the reference solver given identical f, g)
    bool resident_off = false;                  // FRX_RESIDENT=0: one launch per stage from the first round on
    int resident_retry = -1;                    // FRX_RESIDENT_RETRY: its first character, -1 unset
    bool takeover_off = false;                  // FRX_TAKEOVER=0: per-stage rounds run to the end
    bool resident_queue_off = false;            // FRX_RESIDENT_QUEUE=0
    bool host_threads_set = false; int host_threads = 0;   // FRX_HOST_THREADS (atoi): workers of the host-vector plan
    bool zero_copy = true;                      // FRX_ZERO_COPY=0 restores the copies of the host-vector plan
    double round_timeout_ms = 5000.0;           // FRX_ROUND_TIMEOUT_MS: every wait is bounded
    bool dv_geom_set = false; std::string dv_geom;   // FRX_DV_GEOM=E,W,PF,BLK (experiments)
    bool dv_tight = true;                       // FRX_DV_TIGHT=0: history rows of the full 64 W E
    bool mailbox = true;                        // FRX_MAILBOX=0: a round ends when the stream has drained
    int skip_inactive = -1;                     // FRX_SKIP_INACTIVE: -1 unset, 0 begins with '0', else 1
    long drop_round = -1;                       // FRX_DEBUG_DROP_ROUND (atol; fault injection of the tests), -1 unset
    bool trace = false;                         // FRX_TRACE set
};

// ---- decisions ----

// Which failed candidates of a resident plan get a second chance on the per-stage rounds: 0 none, 1 all (diagnostic: FRX_RESIDENT_RETRY=1,
// frx_debug_set_resident_retry), 2 targeted (default: LBFGSERR_INCREASEGRADIENT alone, see plan_route)
constexpr int retry_mode(int first_char, int handle_retry) { return first_char >= 0 ? (first_char == '0' ? 0 : first_char == 't' ? 2 : 1) : (handle_retry != 0 ? 1 : 2); }
constexpr bool wants_retry(int st, int mode) { return st < 0 && st != LBERR_MAXIMUMITERATION && (mode == 1 || (mode == 2 && st == LBERR_INCREASEGRADIENT)); }
// the default keeps the vectors on the device and only the line-search decisions on the host (lbfgs_mode 1: the handle asked for host vectors)
inline bool wants_device_vectors(const PlanSwitches &sw, int lbfgs_mode) { return !sw.lbfgs_host && lbfgs_mode != 1; }
// the resident round kernel first - unless the tests ask for per-stage rounds first, whatever the batch size (frx_debug_set_takeover_at)
inline bool resident_first(const PlanSwitches &sw, int resident_mode, long takeover_at) { return !sw.resident_off && resident_mode != 0 && takeover_at <= 0; }
// large batches: the objective kernels skip candidates that are not being evaluated this round (finished ones above all)
constexpr bool skip_inactive(int sw_skip, int B) { return sw_skip >= 0 ? sw_skip != 0 : B > 64; }

// A batch too large for the resident kernel's clusters runs as per-stage rounds - until no more candidates are left than the chip has clusters for: those continue
// on the resident kernel.  Not when the caller switched the resident kernel, its queue or the take-over off, and not when the resident kernel has just given up on
// this device.  capacity(): resident_capacity(maxXb, CUs), what the resident plan will hold when they are handed over - asked only when everything else permits,
// negative when the device could not be asked.  takeover_at > 0 (tests): also a batch that fits hands over, after so many rounds.
struct TakeOverRule { int capacity = 0; long not_before = 1; };
template <class Cap>
inline TakeOverRule takeover_rule(const PlanSwitches &sw, int resident_mode, bool resident_gave_up, int solver, int knot_threads, int mem_size, int min_n, int B,
                                  long takeover_at, Cap &&capacity) {
    TakeOverRule r;
    const bool wanted = !sw.takeover_off && !sw.resident_off && !sw.resident_queue_off && resident_mode != 0 && !resident_gave_up;
    if (!wanted || solver != SOLVER_KNOT_PCR || knot_threads != 64 || mem_size != 128) return r;
    const int cap = capacity();
    if (cap < 0) return r;
    if (takeover_at > 0) r.not_before = takeover_at;
    if (min_n >= 2 * mem_size && cap >= 1 && (B > cap || takeover_at > 0)) r.capacity = cap;
    return r;
}

// k_lbfgs_pre's geometry (dv_geometry) unless FRX_DV_GEOM names one whose padded row 64 W E holds the longest vector; E == 0: no geometry holds it
struct DvPreGeometry { int E = 0, W = 0, PF = 0, BLK = 4; };
inline DvPreGeometry dv_pre_geometry(int maxXb, const PlanSwitches &sw) {
    DvPreGeometry g;
    dv_geometry(maxXb, &g.E, &g.W, &g.PF);
    int e, w, pf, blk;
    if (sw.dv_geom_set && std::sscanf(sw.dv_geom.c_str(), "%d,%d,%d,%d", &e, &w, &pf, &blk) == 4 && maxXb <= 64 * w * e) { g.E = e; g.W = w; g.PF = pf; g.BLK = blk; }
    return g;
}

// ---- a plan's outcome and what it took ----

// the caller's arrays: x [NX], status [B], and the optional iters, evals, objective [B]
struct PlanArrays { double *x; int *status, *iters, *evals; double *objective; };

struct PlanSnapshot {
    std::vector<double> x, objective;
    std::vector<int> status, iters, evals;
    void save_x(const PlanArrays &a, int NX) { x.assign(a.x, a.x + NX); }
    void save(const PlanArrays &a, int NX, int B) {
        save_x(a, NX);
        status.assign(a.status, a.status + B);
        if (a.iters) iters.assign(a.iters, a.iters + B);
        if (a.evals) evals.assign(a.evals, a.evals + B);
        if (a.objective) objective.assign(a.objective, a.objective + B);
    }
    void restore_x(const PlanArrays &a) const { std::copy(x.begin(), x.end(), a.x); }
    void restore(const PlanArrays &a) const {
        restore_x(a);
        std::copy(status.begin(), status.end(), a.status);
        if (a.iters) std::copy(iters.begin(), iters.end(), a.iters);
        if (a.evals) std::copy(evals.begin(), evals.end(), a.evals);
        if (a.objective) std::copy(objective.begin(), objective.end(), a.objective);
    }
    void reset_candidate(const PlanArrays &a, const int *xoff, int b) const { std::copy(x.begin() + xoff[b], x.begin() + xoff[b + 1], a.x + xoff[b]); }   // x alone
};

// what frx_optimize_stats reports: wall time, the device's and the host's share of it, rounds.  A driver that ran writes all four.
struct PlanTimes {
    double ms = 0.0, ms_dev = 0.0, ms_host = 0.0, rounds = 0.0;
    // a hand-over, or the re-plan after a refused one: the per-stage part before it counts in full
    void add(const PlanTimes &part) { ms += part.ms; ms_dev += part.ms_dev; ms_host += part.ms_host; rounds += part.rounds; }
    // After a second chance on the per-stage rounds; *this: what that run left, `first`: the plan before it, `ran`: the run took place.  A scoped retry (the
    // stragglers of a take-over) reports the sums, or the first plan's figures when it did not run.  An UNSCOPED one reports the sum of the wall times next to the
    // retry run's own device share, host share and rounds (the first plan's own when it did not run): an asymmetry kept as the drivers have always reported it.
    void after_retry(const PlanTimes &first, bool ran, bool scoped) {
        ms = ran ? ms + first.ms : first.ms;
        if (!scoped) return;
        ms_dev = (ran ? ms_dev : 0.0) + first.ms_dev; ms_host = (ran ? ms_host : 0.0) + first.ms_host; rounds = (ran ? rounds : 0.0) + first.rounds;
    }
};

// Stragglers of a per-stage batch that continue on the resident round kernel.  A per-stage round costs four launches whose first is a one-CU recursion over the
// candidate's history (~85 us per round however few candidates are left), a resident round ~25 us - and a batch waits for its slowest candidate (one infeasible
// scenario that wanders 16 673 evaluations held 511 finished ones hostage for a second, profiles/r04_bench_montecarlo4096.json).  When no more than `capacity`
// candidates are still running, the per-stage driver stops and hands them over AS THEY ARE: their solver state machines (the host's side of the plan: line search,
// stop tests, counters), their pending commands, and where their history stands on the device.
struct TakeOver {
    int capacity = 0;                     // in: hand over when at most this many candidates are still running (0: never)
    long not_before = 1;                  // in: ... and this many rounds have run (tests force an early hand-over)
    std::vector<int> cand;                // out: the candidates, in cluster order
    std::vector<SolverDV> sv;             // out: their solvers (pending command inside)
    std::vector<int> newest, bound;       // out: newest slot / number of pairs of their history rows on the device
    std::vector<double> f_last;           // out: objective value of their last evaluation
    PlanTimes spent;                      // out: what the per-stage part took
};

// ---- the route ----

// what the route decides on, as frx_optimize reads it off the handle
struct PlanRouteIn {
    PlanSwitches sw;
    int lbfgs_mode, resident_mode, resident_retry; long takeover_at;
    int solver, knot_threads, mem_size;
    int B, NX; const int *xoff;
};
// the handle's diagnostics of THIS plan, whichever path it takes
struct PlanCounters { int &resident_used, &resident_retried, &resident_failed, &resident_clusters, &taken_over; unsigned long long *spec_counts; };

// Candidates whose plan on the resident kernel ended with an error wants_retry names are planned again on the per-stage rounds, from their start points.  A candidate
// that ends with an L-BFGS error on the resident kernel keeps that verdict, as it would in the reference (lbfgs_optimize returns the code, SE3GCOPTER::optimize
// ignores it, CPU.hpp:1249) - with ONE exception.  The resident kernel forms d = -H g in the compact representation (R^-1 maintained incrementally), the reference by
// the two-loop recursion; in exact arithmetic H is positive definite in both and d is a descent direction.  A search that starts with g.d >= 0
// (LBFGSERR_INCREASEGRADIENT, lbfgs.hpp:766) can therefore only be the work of rounding in the direction itself - an ill-conditioned R - and says nothing about the
// candidate: such candidates, and only those, are planned again on the per-stage rounds, whose direction kernel IS the two-loop recursion.  Line searches that give
// up (-1005, -1007: infeasible corridors, the CPU oracle's verdict as well) are final.
// `scope` (optional): only these candidates are looked at - the stragglers of a take-over, whose dense state was rebuilt on the host by plain back-substitution over
// up to 128 pairs (the long-running, worst-conditioned candidates of a batch).  The first result of a candidate that is planned again is kept: when the per-stage
// path cannot run (its buffers do not fit) it keeps the resident verdict, point and objective instead of ending at its start point.
template <class Paths>
int plan_retry(const PlanRouteIn &in, const PlanArrays &out, PlanCounters &c, PlanTimes &times, const PlanSnapshot &start, const std::vector<int> *scope, Paths &paths) {
    const int mode = retry_mode(in.sw.resident_retry, in.resident_retry);
    std::vector<char> again(in.B, 0);
    int n_again = 0;
    for (int q = 0, n = scope ? (int)scope->size() : in.B; q < n; q++) {
        const int b = scope ? (*scope)[q] : q;
        if (wants_retry(out.status[b], mode)) { again[b] = 1; n_again++; }
    }
    if (n_again == 0) return 0;
    PlanSnapshot first;
    first.save(out, in.NX, in.B);
    for (int b = 0; b < in.B; b++) if (again[b]) start.reset_candidate(out, in.xoff, b);
    const int used = c.resident_used, taken = c.taken_over;
    const PlanTimes t_first = times;
    const int rc = paths.per_stage(&again, nullptr);
    if (rc < 0) return rc;
    if (rc != 0) { first.restore(out); n_again = 0; }
    c.resident_used = used; c.taken_over = taken; c.resident_retried += n_again;
    times.after_retry(t_first, rc == 0, scope != nullptr);
    return 0;
}

// One plan.  Paths: resident(TakeOver *) and per_stage(const std::vector<char> *only, TakeOver *) run the two drivers on `out` and `times` (< 0 an error, 0 done,
// 1 not applicable or given up, per_stage 2: stragglers handed over); device_status() != 0: the resident kernel has just given up on this device; capacity(): see
// takeover_rule; fail(code, text) records an error of the route's own.  Returns < 0 an error, 0 the plan stands in `out`, 1 the caller plans with host vectors from
// the untouched start point.
template <class Paths>
int plan_route(const PlanRouteIn &in, const PlanArrays &out, PlanCounters c, PlanTimes &times, Paths &paths) {
    c.taken_over = 0;
    if (!wants_device_vectors(in.sw, in.lbfgs_mode)) return 1;
    c.resident_used = 0; c.resident_retried = 0; c.resident_failed = 0; c.resident_clusters = 0;
    for (int q = 0; q < 4; q++) c.spec_counts[q] = 0;
    PlanSnapshot start;
    start.save_x(out, in.NX);
    bool resident_gave_up = false;
    if (resident_first(in.sw, in.resident_mode, in.takeover_at)) {
        const int rc = paths.resident(nullptr);
        resident_gave_up = rc != 0 && paths.device_status() != 0;
        if (rc < 0) return rc;
        if (rc == 0) return plan_retry(in, out, c, times, start, nullptr, paths);
        start.restore_x(out);
    }
    int min_n = INT_MAX;
    for (int b = 0; b < in.B; b++) min_n = std::min(min_n, in.xoff[b + 1] - in.xoff[b]);
    const TakeOverRule rule = takeover_rule(in.sw, in.resident_mode, resident_gave_up, in.solver, in.knot_threads, in.mem_size, min_n, in.B, in.takeover_at,
                                            [&] { return paths.capacity(); });
    TakeOver take;
    take.capacity = rule.capacity; take.not_before = rule.not_before;
    const int rc = paths.per_stage(nullptr, take.capacity > 0 ? &take : nullptr);
    if (rc != 2) return rc;
    const PlanTimes part = take.spent;
    const int rc_res = paths.resident(&take);
    if (rc_res < 0) return rc_res;
    if (rc_res == 0) {
        c.taken_over = (int)take.cand.size();
        times.add(part);
        return plan_retry(in, out, c, times, start, &take.cand, paths);      // the stragglers get the resident path's targeted second chance
    }
    // the resident kernel could not take them (another process on the device, a geometry it does not cover): their vectors on the device are no longer the
    // per-stage path's, so they are planned again from their start points, per stage - slower, never wrong
    std::vector<char> again(in.B, 0);
    for (int b : take.cand) { again[b] = 1; start.reset_candidate(out, in.xoff, b); }
    const int rc_again = paths.per_stage(&again, nullptr);
    if (rc_again != 0) return rc_again < 0 ? rc_again : paths.fail(FRX_ERR_HIP, "per-stage path unavailable after a failed take-over");
    c.resident_used = 0;
    times.add(part);
    return 0;
}

} // namespace frx
