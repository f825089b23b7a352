// The geometry of a resident plan (frx_round_kernel.hpp): does the round kernel take this batch, with which chunk size E, how many workgroups per cluster G,
// how many clusters S, through the work queue or not - and the command word the host posts to a cluster.  Plain C++: no HIP and no getenv, so the driver
// (frx_optimize.cpp), the take-over threshold of frx_optimize and the CPU-side enumeration (tests/test_resident_plan_cpu.py) ask the same functions.
#pragma once
#include <algorithm>
#include <cstddef>

#include "frx_device.hpp"
#include "frx_lbfgs.hpp"

namespace frx {

// The environment knobs of a resident plan as read once per plan (resident_knobs_from_env, frx_optimize.cpp); the defaults are the unset variables.
struct ResidentKnobs {
    int e = 0;                                  // FRX_RESIDENT_E: ROUND_E keeps the large chunks
    int g = 0;                                  // FRX_RESIDENT_G: at least this many workgroups per cluster
    bool clusters_set = false; int clusters = 0;   // FRX_RESIDENT_CLUSTERS (experiments / tests): no more than this many clusters; permits the queue
    int queue = -1;                             // FRX_RESIDENT_QUEUE: -1 unset, 0 forbids the work queue, 1 forces it
    int queue_max = 3;                          // FRX_RESIDENT_QUEUE_MAX: x capacity (measured: queue 484 ms against 498 ms per stage at 96 = 3 x 32 candidates, 626 against 514 at 128)
    bool host_threads_set = false; int host_threads = 0;   // FRX_RESIDENT_HOST_THREADS: mailbox service threads
    int scan_pause = 0;                         // FRX_RESIDENT_SCAN_PAUSE: extra pauses between two scans of a thread's mailboxes (experiments)
    int cmd_stride = 4;                         // FRX_RESIDENT_CMD_STRIDE: 4 = one cache line per cluster, 1
    bool fast_control = true, timed_read = false, early_read = true, write_through = false;   // FRX_RESIDENT_FAST_CONTROL=0, _TIMED_READ=1, _EARLY_READ=0, _WRITE_THROUGH=1
    int speculate = 2;                          // FRX_RESIDENT_SPECULATE: 0 | 1 | 2
    bool no_ll20 = false;                       // FRX_RESIDENT_NO_LL20 set
    int stamp_round = 0;                        // FRX_RESIDENT_STAMP_ROUND (with FRX_RESIDENT_PROF)
    double timeout_ms = 5000.0;                 // FRX_ROUND_TIMEOUT_MS
    bool numa = true;                           // FRX_NUMA=0: threads wherever the scheduler puts them
};

// leader + history workgroups (2 E elements of every pair each) + dense: what a candidate of at most maxXb variables needs at chunk size E
inline int resident_workgroups(int maxXb, int E) { return 2 + std::max(1, (maxXb + 2 * E - 1) / (2 * E)); }
// clusters the chip holds at ROUND_E: every workgroup must be resident at once (one per CU; the grid is 8 G ceil(S / 8) blocks)
inline int resident_capacity(int maxXb, int cus) { return 8 * (cus / (8 * resident_workgroups(maxXb, ROUND_E))); }

struct ResidentPlanIn {
    int solver, knot_threads, m, B, Bsel, min_n;   // Bsel candidates run here (a take-over: the stragglers); min_n: the shortest vector among them
    int maxXb, maxN, ppw, cus, resident_mode;
    bool takeover; int dv_mem; bool have_history;  // a take-over continues the per-stage path's history: its length, and whether it exists
};
struct ResidentPlan {
    bool applicable = false;                    // false: the caller runs the one-launch-per-stage path (every other field 0)
    int E = 0, G = 0, S = 0, NXP = 0;
    size_t n_words = 0;                         // RoundLaunch::words
    bool queue = false;                         // S < B: the clusters take the remaining candidates one after the other
};

inline ResidentPlan resident_plan(const ResidentPlanIn &in, const ResidentKnobs &kn) {
    const ResidentPlan no;
    const int B = in.B, Bsel = in.Bsel, m = in.m, cus = in.cus;
    if (in.solver != SOLVER_KNOT_PCR || m < 1 || m > 128 || Bsel < 1) return no;
    if (in.takeover && (in.knot_threads != 64 || m != 128 || in.dv_mem != m || !in.have_history)) return no;   // the take-over instantiation: <= 64 pieces, the stock history length
    // The compact representation inverts R = S^T Y (triangular part); with fewer variables than twice the history length the pairs
    // become linearly dependent and R^-1 loses its digits (n = 1: entries grow like 2^k), where the two-loop recursion of
    // k_lbfgs_pre stays stable.  Such problems (a few pieces) are latency-trivial anyway and take the per-stage rounds.
    if (in.min_n < 2 * m) return no;
    const int blocks8 = (Bsel + 7) / 8;
    // Half the history elements per thread - twice the history workgroups - when the chip has room for them (up to 16 candidates at the headline
    // size; the reference plans ONE): no history register lives in an AGPR then and both history loops are half as long (round 3 measured it
    // on a branch, 31.1 -> 30.3 us per round with one candidate; merged in round 4).  The summation order over the history workgroups, and with
    // it the last bits of a plan, depend on the size class of the batch.  FRX_RESIDENT_E=56 keeps the large chunks.
    const int Gs = resident_workgroups(in.maxXb, ROUND_E_SMALL);
    const int E = kn.e != ROUND_E && Gs <= 16 && (long)8 * Gs * blocks8 <= cus ? ROUND_E_SMALL : ROUND_E;
    const int G_min = resident_workgroups(in.maxXb, E);
    // more workgroups per candidate when the chip has room: the penalty integrand of a candidate is spread over the history workgroups, four wave-tasks each, and
    // the leader - last in line - should get none: it has the adjoint to prepare.  Until round 5 the formula counted the leader as a worker and stopped at 16: the
    // reference's own operating point (ONE candidate, kappa = 48: 64 wave-tasks) ran its penalty share in two passes on 60 waves.  With 18 workgroups (16 x 4 waves,
    // one pass, leader free) a round takes 24.4 instead of 26.4 us, bit-identical plans (scripts/r05/plumbing_g_probe.py: 17 -> 25.6, 20 -> 24.5, 24 -> 25.7).
    const int tasks = (in.maxN + in.ppw - 1) / in.ppw;
    const int want = std::min({(tasks + 3) / 4 + 2, 18, cus / Bsel, cus / (8 * blocks8)});   // (the last bound: the grid is 8 G ceil(B / 8) blocks - a wish that does not fit is not made)
    int G = std::max({G_min, want, kn.g});
    // Every workgroup must be resident at once (one per CU; grid = 8 G ceil(S / 8)).  A batch the chip cannot hold at once runs on
    // S < B clusters that stay on the chip and take the remaining candidates one after the other (work queue: a cluster whose candidate is
    // finished gets the next one with its DV_NEXT command instead of DV_QUIT).  The clusters run independently, so the batch takes
    // ~sum(evaluations) / S rounds where the per-stage path - every candidate in every launch - takes max(evaluations) rounds of a
    // launch that grows with B: measured (profiles/r03_queue_sizes.jsonl) the queue wins up to a few times the chip's capacity, the
    // per-stage path beyond; resident_mode 2 / FRX_RESIDENT_QUEUE=1 force the queue, FRX_RESIDENT_QUEUE=0 forbids it.
    int S = Bsel;
    // (the small chunks are only chosen when all Bsel clusters fit at G_min, and the capacity at ROUND_E is no smaller than theirs: one formula serves both sizes)
    if ((long)8 * G * blocks8 > cus) { G = G_min; S = std::min(Bsel, resident_capacity(in.maxXb, cus)); }
    const bool capped = !in.takeover && kn.clusters_set;
    if (capped) S = std::min(S, std::max(1, kn.clusters));
    if (S < 1) return no;
    if (in.takeover && S < Bsel) return no;                                          // a take-over has one cluster per straggler (no queue)
    const bool queue = S < B && !in.takeover;
    if (queue && !(kn.queue >= 0 ? kn.queue != 0 : (capped || in.resident_mode == 2 || B <= kn.queue_max * S))) return no;
    ResidentPlan pl;
    pl.applicable = true; pl.E = E; pl.G = G; pl.S = S; pl.queue = queue;
    pl.NXP = (G - 2) * 2 * E;
    pl.n_words = (size_t)ROUND_WORDS_PER_CAND * S + 2 + (size_t)S * G + 4 * (size_t)B;
    return pl;
}

// host -> device: word = seq << 32 | bound << 20 | slot << 8 | flags (frx_round_kernel.hpp, RoundCmd).  DV_STEP_IS_ONE lets the leader confirm a predicted
// command from this word alone; a trial inside a search (TRIAL without ADVANCE) has no use for slot and pair count: a fold of the step's bits rides in their place.
inline unsigned long long round_command_word(unsigned long long seq, int flags, int slot, int bound, double step) {
    if (step == 1.0 && !(flags & (DV_QUIT | DV_NEXT))) flags |= DV_STEP_IS_ONE;
    if ((flags & DV_TRIAL) && !(flags & DV_ADVANCE)) {
        const unsigned h = dv_step_hash(step);
        slot = (int)(h & 0xFFFu); bound = (int)(h >> 12);
    }
    return (seq << 32) | ((unsigned long long)(bound & 0xFFF) << 20) | ((unsigned long long)(slot & 0xFFF) << 8) | (unsigned long long)(flags & 0xFF);
}

} // namespace frx
