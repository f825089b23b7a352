// ONE LAUNCH PER EVALUATION for batches the chip holds at once (frx_objective_eval[_device]: x -> (f, grad f), SURVEY.md 8 row a1;
// the reference's objectiveFunc, se3gcopter_cpu.hpp:961-1000, which its CUDA path splits over a host call, one persistent kernel and a host call again,
// cuda_computer.cu:530-547).
//
// The three stage kernels of an evaluation (forward map, penalty integral, adjoint) are three dependent launches: at the headline batch
// (32 candidates x 64 pieces) each is one wave's dependent chain of 4.6-7.7 us of which 1.5-2.5 us are the launch itself - start of the grid,
// the first trip to HBM for operands the previous kernel just had in LDS, the drain at the end (the same bodies inside the resident round kernel,
// frx_round_kernel.hpp, take 5.2 / 3.1 / 5.2 us).  Here an evaluation is one grid of CLUSTERS, one per candidate:
//   every workgroup   runs the forward map on the same x (forward_knot_body, MODE 5: x and the polytopes staged into its own LDS, (C, T) kept there, nothing to global memory),
//                     so (C, T) never travel between workgroups.  Early-duration form (ET, the default; FRX_EVAL_EARLY_T=0 takes the staged form): wave 0 - the matrix
//                     wave - loads tau into registers as its first loads and forms the durations on its own, waves 1-3 stage xi and the polytopes (PRE below: without a
//                     test per element; FRX_EVAL_PRELUDE=0 takes the form before); one early barrier
//                     (counters zeroed, the status word broadcast) and the barrier in front of the coefficient collection are the only workgroup barriers of the forward map
//   workgroup 0       LEADER: then everything of the adjoint that does not need the penalty partials (ADJ below: the waypoint layer's operands and scale factors too),
//                     polls the partials, finishes the adjoint, writes f and the gradient
//   workgroups 1..G-1 MEMBERS, every WAVE on its own behind the forward map: the corridor blocks of its wave-task (ppw pieces; loaded behind the forward map's own loads,
//                     in flight under it), the penalty samples out of the workgroup's (C, T) copy, the 20 partials per piece out as self-validating granules
//                     (rk_ll_put, frx_kernels.hpp: no drain, no flag behind the payload) and leave
// Same integrand and sums as the stage kernels (f is bit-identical; both forms of the forward map too); the adjoint runs in the resident order of operations
// (backward_knot_wsp64), whose gradient differs from the stage kernel's in the last bits (<= 1e-11 relative, tests/test_gpu_parity.py).
//
// Tags instead of zeroed buffers: the launch is captured in hipGraphs (bench.py replays one), so nothing on the host may run between two of them.  Every
// cluster keeps the tag of its last COMPLETED evaluation in device memory (`done`); an evaluation uses tag = done + 1 for its flag and its granules, and thread 0
// of the leader stores it back from inside the adjoint, next to f (EvalTail, frx_kernels.hpp).  That store is behind the workgroup barrier that follows the knot
// adjoint, and every lane that polls the partials is in front of that barrier: `done` moves behind the arrival of every partial, hence behind every member's read
// of it (a member without a task reads nothing and leaves).  Nothing else orders on `done` within a launch - the axis waves' gradient stores that are still in
// flight when it leaves belong to the same kernel, and the next reader of either is a later launch.  Launches on one stream do not overlap, so no workgroup
// ever sees a tag of the future.  The verdict - did a wait of this leader end without its partials - comes out of a word of the leader's LDS that the polling
// lanes set next to their CAS on the global word; a word left by an EARLIER launch is caught at entry, and a code another cluster's leader sets during this launch
// concerns that cluster's f alone (it is NaN, and the host word carries the code).  The leader's tail therefore has no load and no barrier: f, `done` and the
// gradient's last stores are in flight together (the form before: FRX_EVAL_TAIL=0, 0.64 us between wave 0's last store and `done` on the stamps).
// Every spin is bounded (EvalClusterArgs::timeout_ticks); an expired wait records RK_ERR_PHASE / RK_ERR_ARRIVE in `status` and the candidate's f becomes NaN.
// Residency: a leader waits for members of the SAME launch, so all of a cluster's workgroups have to get a CU.  Blocks are dispatched in index order and a
// cluster's blocks are 8 apart within one group of 8 G consecutive blocks (the XCD mapping of k_round), so the resident blocks of a launch always contain
// whole clusters, which finish and make room; the launcher only takes this path when B G <= the device's CU count (frx_device.hip).
#pragma once
#include <type_traits>

#include "frx_eval_front.hpp"
#include "frx_round_kernel.hpp"

namespace frx {

// The three leading lines of the argument block (FR below): every pointer and integer that an ADDRESS of the front's loads, or the LDS layout, is made of, the time layer's two
// switches, and in the third line the run-time VALUES the geometry class parks in vector registers across the forward map (the other instantiations do not read that line) -
// copies of fields of `dp` and of the geometry further down, which keep their places (DevProblem is every other kernel's too).
struct EvalArgsLead {
    const int *piece_coarse, *piece_iv, *wp_nv, *wp_vbeg, *wp_xbeg;
    const double *vrec, *hblk, *headPVA, *tailPVA;
    unsigned *status, *words;
    int maxN19, maxXb, maxVb, maxCN, nsteps, pen_lds, ppw, Kmax, soft, c2;
    double chi[4], inv_kappa; ll_u64 *out20ll; int kappa, pad[3];
};
static_assert(sizeof(EvalArgsLead) == 192 && offsetof(EvalArgsLead, chi) == 128, "three 64-byte lines");

struct EvalClusterArgs {                      // constant for the life of a handle (a copy lives in device memory: ARGP below)
    EvalArgsLead lead;
    DevProblem dp;
    double *T, *C;
    ll_u64 *out20ll;                         // 20 granules per piece: the penalty partials, members -> leader (its own buffer: the round kernel's carries tags of its own).  Candidate c owns the 40 N words
                                             // behind 40 poff[c]; in them granule (value v, piece k) lies at word 2 (v N + k) - value-major, the order the leader's lanes poll in (HO below) - or, in the
                                             // piece-major form, at 2 (20 k + v).  One form for the life of a handle: a tag validates a word only at the address it was written for
    unsigned *words;                         // [B][64]: cluster k's 256-byte block: word 0 = gate (tag << 4 | the leader's XCD + 1: (C, T) are out), words 8 .. 8 + G - 2 = tag << 4 | XCD + 1 of
                                             // members 1 .. G-1 (written at their entry), word 32 = tag of the last completed evaluation
    unsigned *status;                        // [1] sticky error word
    int G, maxCN, maxXb, maxVb, nsteps, lpp, ppw, Kmax, pen_lds, maxN19;
    const EvalFront *front;                  // [B] front records (frx_eval_front.hpp), a device allocation of the handle; a launch passes it as the kernel's third argument
};
static_assert(offsetof(EvalClusterArgs, lead) == 0, "the leading lines lead");

// LDS of a workgroup (doubles): 2 control | (C, T) copy, x, polytopes, multipliers, waypoint sums, evaluation scratch (leader AND members: both run the forward map) | members: 4 waves x pen_lds
struct EvalClusterLds { int ctl, xs, vs, pw, wq, ev, mem, total; };
__host__ __device__ inline EvalClusterLds eval_cluster_lds(int maxN19, int maxXb, int maxVb, int maxCN, int nsteps, int pen_lds) {
    EvalClusterLds L;
    int o = 2;
    L.ctl = o; o += (maxN19 + 1) & ~1;
    L.xs = o; o += (maxXb + 1) & ~1;
    L.vs = o; o += (maxVb + 1) & ~1;
    L.pw = o; o += ((nsteps * 8 + 5) * 64 + 1) & ~1;
    L.wq = o; o += 4 * 64;
    L.ev = o;
    const int e = 36 * 64 + 9 * 65 + 2 * 64 + maxCN + 16;   // rows | knot arrays | Tf, gT | gCo | cross-wave partials (forward_knot_body / backward_knot_wsp64 with resident operands)
    o += (e + 1) & ~1;
    L.mem = o;                                                          // members (round 6: they run the forward map themselves, in the leader's layout): 4 waves x pen_lds behind it
    L.total = o + 4 * pen_lds + 8;
    return L;
}

// ARGP (round 6): the arguments that are constant for the life of a handle - the problem descriptor and the geometry, ~400 bytes - come
// through a POINTER to a copy in device memory instead of by value, and only what changes per call (x, f, g, the bound, the test switches) stays in the kernarg
// segment.  By value every field is loaded into a scalar register at entry and stays live for the whole kernel: 100 registers' worth of them for a budget of 102 -
// the shipped object had 63 SGPR spills and 767 v_readlane reloads in front of their uses (scripts/isa_report.py).  Behind a pointer a field is an s_load at its
// use (scalar cache) and nothing is kept: 0 spills, 12 v_readlane, 3463 instead of 4093 VALU instructions in the kernel.
struct EvalCallArgs {                         // what changes per call
    const double *x; double *f, *g;
    unsigned *status_host;                   // optional, mapped host memory: the code of an expired wait, where the launcher sees it without a synchronisation (frx_api.cpp: launch_eval)
    rk_u64 timeout_ticks;                    // bound of every spin
    unsigned short G, B;                     // (FR) the handle's G and B - with them and the records' pointer (the kernel's third argument) a workgroup knows its cluster, its place in it and its
                                             // record's address from the kernarg segment alone.  Handle constants, so a captured graph may hold them; B G <= the CU count is the launcher's rule
    unsigned char test_drop_members;         // tests (frx_debug_set_eval_fused(p, 2)): the members leave at once, as if they never got a CU - the leader's wait for the partials expires
    unsigned char force_wt;                  // 1 = every payload store write-through, as if no two workgroups shared an XCD (tests: FRX_EVAL_FUSED_WT=1)
};
static_assert(sizeof(EvalCallArgs) + 2 * sizeof(void *) <= 64, "argument pointer, call arguments and the records' pointer: one 64-byte line of the kernarg segment");
// The early barrier of the early-duration form (forward_knot_body<.., ET>): the caller's loads behind the body's, then one barrier that zeroes the counters and makes the
// status early-out workgroup-uniform.
// FRN (FR below): the caller has issued wave 0's tau load itself and holds what the early-duration block otherwise reads from the index tables and the argument block.
// PRN (PRE below): the shortened prelude of the forward map.
template <class F, bool NS = false, bool FRN = false, bool PRN = false> struct EvalEarlySync {
    static constexpr bool nostamps = NS;          // (CH below: no cycle stamps compiled into the forward map)
    static constexpr bool front_held = FRN;
    static constexpr bool prelude = PRN;
    const F &f; long long *st; bool steps;
    long long *front;                             // (cluster 0's leader, stamped form) [0] wave 0's tau load issued, [1] tau in its register: slots 32, 33 of the stamp block
    // (FRN) the candidate's tau / variable / vertex-double counts, the time layer's two switches, the candidate's first vertex record, wave 0's tau
    int nT, nx, nvd, soft, c2; gptr<const double> vsrc; double tau;
    long long *pst = nullptr;                     // (cluster 0's leader and its last member with a task, stamped form) the prelude's stamps, stretch by stretch: forward_knot_body
    __device__ __forceinline__ bool sync() const { return f(); }
};
// TAIL (the default; FRX_EVAL_TAIL=0 takes the other form, A/B): thread 0 of the leader stores f and `done` inside the adjoint, right behind the objective's sum
// (EvalTail, frx_kernels.hpp); otherwise behind a workgroup barrier and a load of the global status word at the kernel's end, as until now.
// HO (the default; FRX_EVAL_HANDOFF=0 takes the other form, A/B; with the tail above and the argument pointer only): the hand-off of the partials laid out for its reader
// (EvalHandoff, frx_kernels.hpp) - the members store a granule with one 16-byte store at its value-major place; the leader's waves poll with one coalesced 16-byte load
// per granule, wave 0 two and an axis wave six, and the axis waves request the 52 multipliers of their knot in front of the poll instead of behind it.
// CH (the default; FRX_EVAL_CHAIN=0 takes the other form, A/B; with the three above only): the PRODUCTION instantiation.  The cycle stamps are a compile-time property - no
// read of a clock, no load of the stamps pointer, no branch on it in this kernel or in the bodies it calls (the diagnostics, frx_debug_profile_eval_cluster and the
// timeline scripts, launch the CH = false instantiation with an argument block of their own that carries the pointer: launch_eval_cluster picks both by the handle's
// stamps pointer).  And no argument load behind a wait of the chain: behind the argument pointer every field is a scalar load at its use, and the wait for it (lgkmcnt)
// drains the LDS reads of the lone wave around it.  What the stretches behind the forward map read is loaded ONCE and pinned in scalar registers (as_uniform, frx_kernels.hpp) -
//   leader, in front of the adjoint's set-up (so in front of the poll, where it idles): rho, the fixed-time layer's soft / c2 / sumT, the gradient's and f's base, `done`, status_host (EvalChain, EvalTail);
//   members, in front of the samples: lpp, N, the task's first piece, the candidate's granule base;
//   members too: the four penalty weights, each of which is otherwise read inside the branch of its violated constraint, in the middle of a lane's samples;
//   every workgroup, in front of the forward map: nsteps (the axis waves read it behind the last reduction step).
// GEO (EvalGeomK16; FRX_EVAL_GEOM=0 takes the other form, A/B; with the switches above at their defaults only): the GEOMETRY CLASS of the headline handle as integer constants -
// kappa + 1 = 17 lanes per piece, 3 pieces per wave-task, corridor blocks of Kmax = 8 half-spaces (36 doubles), six reduction steps.  The kernel otherwise takes all of
// them as run-time integers behind the argument pointer, and on a member's path between the forward map's last barrier and its first sample that is about 230
// instructions: scalar loads in five groups with a wait each, a division for lane / lpp, a four-way predicated staging scaffold with a second-trip loop, multiplies by
// strides.  With the class
//   the lane -> (piece, sample) map, the task's first piece, the block stride and the per-wave LDS are constants, and with lpp and Kmax constant where they are inlined
//   the sample loop, the half-space chunks and penalty_reduce's block of sixteen reads fold to the trips they take;
//   a task's corridor blocks (at most 54 double2) are ONE load per lane and one LDS store behind the forward map;
//   what the samples and the granule stores still read from the argument block (the four weights, kappa, 1 / kappa: run-time VALUES, as before; the candidate's granule
//   base) is loaded in front of the forward map and kept in VECTOR registers across it (the kernel uses 232 of 512; the forward map and the samples have the scalar
//   registers to themselves): the samples take the weights and kappa as vector operands, the granule base moves to a scalar pair in front of the samples.
// N stays per candidate (ragged handles qualify), and so does everything that is not an integer of the geometry: no floating-point expression, operand or order changes,
// f and the gradient are the run-time form's bits (tests/test_gpu_eval_geometry.py).  launch_eval_cluster picks the class instantiation when the handle's geometry equals
// it exactly; both CH values have one, so the diagnostics stamp the form that is timed.  The number of reduction steps belongs to the class (it selects the handles) but
// reaches the bodies as an opaque scalar: folded into forward_knot_body / backward_knot_wsp64, and with the six steps of the matrix and axis waves unrolled on top, the
// evaluation measured no faster and slower respectively (profiles/NOTES.md), so the bodies of frx_kernels.hpp compile as they do for everybody else.
struct EvalGeomK16 { static constexpr int LPP = 17, PPW = 3, KMAX = 8, NSTEPS = 6; };
template <class GEO> struct eval_geom {
    static constexpr bool fixed = true;
    static constexpr int lpp = GEO::LPP, ppw = GEO::PPW, kmax = GEO::KMAX, nsteps = GEO::NSTEPS;
    static constexpr int hstride = (kmax + 1) * 4, pen_lds = ppw * 19 + ppw * hstride + 64 * 21;
    static_assert(ppw * lpp <= 64 && ppw * hstride <= 2 * 64, "a wave-task: one lane per sample, one double2 of its corridor blocks per lane");
};
template <> struct eval_geom<void> { static constexpr bool fixed = false; static constexpr int lpp = 0, ppw = 0, kmax = 0, nsteps = 0, hstride = 0, pen_lds = 0; };
// FR (the default wherever the form has the argument pointer and early durations; FRX_EVAL_FRONT=0 takes the other front, A/B): TWO trips behind the entry.  Through the
// tables the front is a chain of first touches, each waited for before the next address exists: the argument block's lines one by one, poff, coff / xoff / cvoff, the
// per-piece and waypoint tables, the end states, the class's parked values - and only then tau (2.0 us from the leader's entry to the tau load on the stamps,
// profiles/NOTES.md).  Here the kernarg segment alone gives a workgroup its cluster and its place in it (G and B travel in EvalCallArgs, the records' pointer is the
// kernel's third argument); it reads its candidate's record (EvalFront, one line) and the three leading lines of the argument block (EvalArgsLead) as one group of scalar
// loads, waits ONCE, and issues every global load of the front as one group: the status word and `done` (neither is waited for in front of the barrier by anybody but
// thread 0's wave), wave 0's tau, the piece and waypoint tables' entries, the end states - the body receives them as a KnotPre - then the body's own first staging trip
// and the members' corridor block.  The class's parked values come with the third leading line: requested behind the loads they would be a trip of their own, waited
// for at the early barrier.  Integers only: no floating-point expression, operand or order changes, f and the gradient are the other front's bits
// (tests/test_gpu_eval_front.py).  The read of the broadcast status word behind the early barrier is an LDS read by type here (as a generic volatile read it is a flat load
// with a wait for every load the wave has in flight).
// PRE (the default wherever the form has the two-trip front and the value-major hand-off; FRX_EVAL_PRELUDE=0 takes the prelude before, A/B): the forward map's axis waves
// stage xi and the polytopes without a test per element (forward_knot_body<.., ET>, ES::prelude: frx_kernels.hpp) - all 256 workgroups run that stretch, between the
// early barrier and the waypoint map, so it is on every workgroup's chain.  Measured 12.26 -> 11.89 us per evaluation (profiles/NOTES.md); three further steps on the
// same two chains - a member's wave 0 requesting its corridor block behind the durations, the Hermite operands under the wait for the last reduction step, the axis
// waves' step gate without its sleep - measured level or slower on top of it and are not in the tree.  The stamped instantiation (CH = false) of either prelude carries
// the stamps of both chains stretch by stretch: slots 80..110, frx_debug_profile_eval_forward.
// ADJ (the default wherever the shortened prelude is on; FRX_EVAL_ADJOINT=0 takes the adjoint before, A/B): the LEADER's adjoint gets the waypoint layer's operands in
// front of the poll (EvalHandoff<.., AJ>, backward_knot_wsp64: frx_kernels.hpp).  From the poll to the end of the kernel only the leader works, so whatever stands
// behind the poll is on the only chain there is; between the solve and the barrier behind the knot adjoint every axis lane requested forty LDS reads, read the forward
// map's four sums and divided - none of which depends on a partial.  They are requested next to the 52 multipliers instead, where the leader waits anyway; behind the
// solve only the dozen operations on mu remain in front of the barrier (0.64 -> 0.40 us on the stamps).  The place of loads only: f and the gradient are the other
// form's bits (tests/test_gpu_eval_adjoint.py).  Measured 11.90 -> 11.43 us per evaluation (profiles/NOTES.md); the adjoint's top out of the front's registers instead
// of through the offset tables, built with it, measured 0.08 us SLOWER on its own and is not in the tree.
template <bool ARGP, bool ET, bool TAIL = true, bool HO = false, bool CH = false, class GEO = void, bool FR = false, bool PRE = false, bool ADJ = false>
__global__ __launch_bounds__(256, 1) void k_eval_cluster(typename std::conditional<ARGP, const EvalClusterArgs *__restrict__, EvalClusterArgs>::type arg, EvalCallArgs call,
                                                         const EvalFront *__restrict__ front) {   // (front: a kernel argument of its own - through a restrict pointer to const the record is a scalar load)
    static_assert(!CH || (ARGP && TAIL && HO), "the production form: argument pointer, inline tail, value-major hand-off");
    typedef eval_geom<GEO> GC;
    constexpr bool GF = GC::fixed;
    static_assert(!GF || (ARGP && ET && TAIL && HO), "the geometry class: the default form of every other switch");
    static_assert(!FR || (ARGP && ET), "the two-trip front: the argument pointer and early durations");
    static_assert(!PRE || (FR && HO), "the shortened prelude: the two-trip front and the value-major hand-off");
    static_assert(!ADJ || PRE, "the adjoint's operands in front of the poll: where the shortened prelude is on");
    const EvalClusterArgs &a = [&]() -> const EvalClusterArgs & { if constexpr (ARGP) return *arg; else return arg; }();
    const auto stp = [&]() -> long long * { if constexpr (CH) return nullptr; else return a.dp.stamps; };   // (CH: a constant - every stamp below folds away)
    extern __shared__ __attribute__((aligned(16))) double sm[];
    long long fr_entry = 0, fr_entry_cyc = 0;                       // (FR, stamped form: the clocks are read in front of the first load, the stamps go out once their pointer is there)
    if constexpr (FR && !CH) { fr_entry = (long long)wall_clock64(); fr_entry_cyc = (long long)__builtin_readcyclecounter(); }
    const int lane8 = blockIdx.x & 7, rest = blockIdx.x >> 3;
    const int nG = [&]() -> int { if constexpr (FR) return call.G; else return a.G; }();
    const int wg = rest % nG, k = lane8 + 8 * (rest / nG);         // (k_round's mapping: a cluster's blocks share blockIdx % 8 - one XCD, as observed)
    if (k >= [&]() -> int { if constexpr (FR) return call.B; else return a.dp.B; }()) return;
    const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int c = k;
    // (FR) the first trip: the candidate's record and the leading lines, one group of scalar loads and one wait
    EvalFront fr = {};
    EvalArgsLead ld = {};
    gptr<const int> l_pc = nullptr, l_piv = nullptr, l_wnv = nullptr, l_wvb = nullptr, l_wxb = nullptr;
    gptr<const double> l_vrec = nullptr, l_hblk = nullptr, l_head = nullptr, l_tail = nullptr;
    gptr<unsigned> l_status = nullptr, l_words = nullptr;
    if constexpr (FR) {
        fr = front[k]; ld = a.lead;
        l_pc = (gptr<const int>)ld.piece_coarse; l_piv = (gptr<const int>)ld.piece_iv; l_wnv = (gptr<const int>)ld.wp_nv; l_wvb = (gptr<const int>)ld.wp_vbeg; l_wxb = (gptr<const int>)ld.wp_xbeg;
        l_vrec = (gptr<const double>)ld.vrec; l_hblk = (gptr<const double>)ld.hblk; l_head = (gptr<const double>)ld.headPVA; l_tail = (gptr<const double>)ld.tailPVA;
        l_status = (gptr<unsigned>)ld.status; l_words = (gptr<unsigned>)ld.words;
        // (one statement: the loads go out together in front of it.  The class reads its geometry's integers from no line, and its parked values from the third)
#define FRX_FRONT_PINS "+s"(fr.p0), "+s"(fr.N), "+s"(fr.c0), "+s"(fr.cN), "+s"(fr.x0), "+s"(fr.nx), "+s"(fr.nT), "+s"(fr.cv0), "+s"(fr.nvd), "+s"(fr.wbase), "+s"(fr.ntasks), \
                        "+s"(l_pc), "+s"(l_piv), "+s"(l_wnv), "+s"(l_wvb), "+s"(l_wxb), "+s"(l_vrec), "+s"(l_hblk), "+s"(l_head), "+s"(l_tail), "+s"(l_status), "+s"(l_words), \
                        "+s"(ld.maxN19), "+s"(ld.maxXb), "+s"(ld.maxVb), "+s"(ld.maxCN), "+s"(ld.soft), "+s"(ld.c2)
        if constexpr (GF) asm volatile("" : FRX_FRONT_PINS, "+s"(ld.chi[0]), "+s"(ld.chi[1]), "+s"(ld.chi[2]), "+s"(ld.chi[3]), "+s"(ld.inv_kappa), "+s"(ld.kappa));
        else asm volatile("" : FRX_FRONT_PINS, "+s"(ld.nsteps), "+s"(ld.pen_lds), "+s"(ld.ppw), "+s"(ld.Kmax));
#undef FRX_FRONT_PINS
    }
    // (diagnostic, frx_debug_profile_eval_cluster: cycle stamps of cluster 0 - 40..43 the leader: entry, forward map done, adjoint done, end; 32, 33 wave 0's tau load issued / tau in its register, see forward_knot_body; 64..68 its tail, see EvalTail; 70..76 its poll for the partials, see EvalHandoff; 44..48 wave 0 of member 1, see penalty_wave_ll, and 69: the gate word's value has arrived - these in ticks of the 100 MHz counter all workgroups share; 49: the leader's shader clock at entry, the origin of the bodies' own stamps 0..31)
    if constexpr (FR) { if (stp() && k == 0 && wg == 0 && t == 0) { stp()[40] = fr_entry; stp()[49] = fr_entry_cyc; } }
    else
    if (stp() && k == 0 && wg == 0 && t == 0) { stp()[40] = (long long)wall_clock64(); stp()[49] = (long long)__builtin_readcyclecounter(); }
    unsigned *flag = FR ? (unsigned *)l_words + (size_t)k * 64 : a.words + (size_t)k * 64, *done = flag + 32;
    const int p0 = [&]() -> int { if constexpr (FR) return fr.p0; else return a.dp.poff[c]; }();
    const int N = [&]() -> int { if constexpr (FR) return fr.N; else return a.dp.poff[c + 1] - p0; }();
    // (the geometry's integers: constants of the class, or the argument block's fields read at each use as before; FR: in front of the forward map the leading lines' copies)
    const auto g_ppw = [&]() -> int { if constexpr (GF) return GC::ppw; else return a.ppw; };
    const auto g_pen_lds = [&]() -> int { if constexpr (GF) return GC::pen_lds; else return a.pen_lds; };
    const auto g_kmax = [&]() -> int { if constexpr (GF) return GC::kmax; else return a.Kmax; };
    const auto f_ppw = [&]() -> int { if constexpr (GF) return GC::ppw; else if constexpr (FR) return ld.ppw; else return a.ppw; };
    const auto f_pen_lds = [&]() -> int { if constexpr (GF) return GC::pen_lds; else if constexpr (FR) return ld.pen_lds; else return a.pen_lds; };
    const auto f_kmax = [&]() -> int { if constexpr (GF) return GC::kmax; else if constexpr (FR) return ld.Kmax; else return a.Kmax; };
    const int ntasks = [&]() -> int { if constexpr (FR) return fr.ntasks; else return (N + g_ppw() - 1) / g_ppw(); }();   // wave-tasks of this candidate: ppw pieces each; members 1 .. G-1 hold 4 (G - 1) >= ntasks waves
    if (wg != 0 && ((wg - 1) * 4 >= ntasks || call.test_drop_members)) return;   // a member without a task
    unsigned st0 = 0u;                                              // (ET: thread 0's copy of the status word, the workgroup's first load)
    if constexpr (FR) { if (t == 0) st0 = __hip_atomic_load(l_status, FRX_RLX_AGENT); }
    else
    if constexpr (ET) { if (t == 0) st0 = __hip_atomic_load(a.status, FRX_RLX_AGENT); }
    else {
    // A wait of an EARLIER launch expired and nobody has cleared the word yet (the capturable form has no host-synchronous point of its own: replays of a captured
    // graph go on until the caller polls frx_eval_status): nothing is evaluated, nothing spins; the objective values say so.
    if (__builtin_expect(__hip_atomic_load(a.status, FRX_RLX_AGENT) != 0u, 0)) {
        if (wg == 0 && threadIdx.x == 0) call.f[k] = __builtin_nan("");
        return;
    }
    }
    // (stays in a vector register: nothing waits for the load until the tag is used.  FR: behind a global address the compiler knows to be uniform it would move the value to a scalar
    // register at once, with a wait for every load in front of tau - so the load goes through an offset of zero it does not know, and the tag is formed behind the early barrier)
    unsigned tag = 0u, tag_v = 0u;
    if constexpr (FR) { int tag_at = 0; asm volatile("" : "+v"(tag_at)); tag_v = __hip_atomic_load(done + tag_at, FRX_RLX_AGENT); }
    else {
    tag = __hip_atomic_load(done, FRX_RLX_AGENT) + 1u;
    if (tag >= (1u << 28)) tag = 1u;
    }
    // Where does this workgroup run?  Payload between two workgroups of one XCD can meet in that XCD's L2 (plain stores, L1-bypassing loads); across XCDs it has
    // to be written through to memory - measured 2.1 us of an 18.5 us evaluation.  The block -> cluster mapping above puts a cluster on one XCD on the hardware
    // this was written on, but nothing relies on it: the members publish their XCD at entry, the leader compares before it sends (C, T), its own XCD travels in
    // the gate word, and whoever finds a partner elsewhere (or not yet heard of) writes through.
    unsigned my_xcc = 0;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(my_xcc));
    my_xcc = call.force_wt ? 0u : (my_xcc & 7u) + 1u;                  // 0: "nowhere" - never equal to a partner's
    int nsteps = GC::nsteps;
    if constexpr (!GF) { if constexpr (FR) nsteps = ld.nsteps; else nsteps = a.nsteps; }
    if constexpr (CH || GF) asm volatile("" : "+s"(nsteps));            // (GEO: the class's constant, opaque in a scalar register - see above)
    const EvalClusterLds L = FR ? eval_cluster_lds(ld.maxN19, ld.maxXb, ld.maxVb, ld.maxCN, nsteps, f_pen_lds()) : eval_cluster_lds(a.maxN19, a.maxXb, a.maxVb, a.maxCN, nsteps, g_pen_lds());
    // Round 6: the MEMBERS run the forward map too - the same body on the same x, so their (C, T) are the leader's bit for bit - instead of waiting for the leader's
    // coefficients: until now (C, T) travelled as granules behind a gate word (sweep 0.7 us, gate seen 0.15, granules polled and staged 0.7 us on the members' side) while
    // the members' four waves had nothing to do for the first 8 us of the launch.  The leader sends nothing; its XCD goes into the gate word at ENTRY (the members look at
    // it when their partials leave, microseconds later; not there yet counts as "elsewhere": write-through).
    double *ctl = sm + L.ctl, *ev = sm + L.ev;
    const lds_vuptr verdict = (lds_vuptr)(unsigned *)sm;                              // (leader) a wait for the penalty partials ended without them: EvalTail.  Zeroed in front of the forward map's barriers
    ResidentOps ro;
    ro.xs = sm + L.xs; ro.vs = sm + L.vs; ro.dsv = sm + L.xs; ro.pw = sm + L.pw; ro.gs = nullptr; ro.vskew = 0; ro.wq = sm + L.wq; ro.gpub = nullptr; ro.gwt = true;
    ro.quiet = wg != 0;
    const int task = (wg - 1) * 4 + wave;                                  // (members) this wave's task: ppw pieces
    const bool has_task = wg != 0 && task < ntasks;
    const int gp0 = p0 + task * f_ppw(), npieces = has_task ? min(f_ppw(), N - task * f_ppw()) : 0;
    const int hstride = (f_kmax() + 1) * 4;
    double *wsm = sm + L.mem + (size_t)wave * f_pen_lds(), *hS = wsm, *red = wsm + (size_t)f_ppw() * hstride;
    double2 hv[4];                                                  // (ET, members) the first trip of the corridor blocks, loaded behind the forward map's loads
    const double2 *h2 = (const double2 *)((FR ? (const double *)l_hblk : a.dp.hblk) + (size_t)gp0 * hstride);
    const int nh2 = (npieces * hstride) >> 1;
    bool bad = false;
    // (GEO, members) the run-time values the samples read from the argument block: requested here, parked in vector registers across the forward map
    double m_chi[4] = {0.0, 0.0, 0.0, 0.0}, m_invk = 0.0; int m_kappa = 0;
    gptr<ll_u64> m_llv = nullptr;
    if constexpr (GF) {
#pragma unroll
        for (int i = 0; i < 4; i++) m_chi[i] = FR ? ld.chi[i] : a.dp.pc.chi[i];         // (FR: they came with the leading lines - no trip of their own)
        m_invk = FR ? ld.inv_kappa : a.dp.inv_kappa; m_kappa = FR ? ld.kappa : a.dp.kappa;
        m_llv = (gptr<ll_u64>)((FR ? ld.out20ll : a.out20ll) + (size_t)p0 * 40);
        asm volatile("" : "+v"(m_chi[0]), "+v"(m_chi[1]), "+v"(m_chi[2]), "+v"(m_chi[3]), "+v"(m_invk), "+v"(m_kappa), "+v"(m_llv));
    }
    if constexpr (ET) {
        if (k == 0 && wg == 1 && wave == 0 && lane == 0 && stp()) stp()[44] = (long long)wall_clock64();
        const int wg_last = min(nG - 1, (ntasks - 1) / 4 + 1);            // the last-dispatched member with a task
        long long *pst = nullptr;                                   // (the prelude's stamps: slots 80.. of cluster 0's leader and of its last member with a task)
        if constexpr (!CH) { if (stp() && k == 0 && (wg == 0 || wg == wg_last)) pst = stp() + 80; }
        const auto early = [&]() -> bool {
            if (has_task) {
                if constexpr (GF) hv[0] = h2[lane < nh2 ? lane : nh2 - 1];          // (nh2 <= 54: the one trip there is)
                else {
#pragma unroll
                for (int u = 0; u < 4; u++) { const int i = lane + 64 * u; hv[u] = h2[i < nh2 ? i : nh2 - 1]; }
                }
            }
            unsigned *w = (unsigned *)(ev + 24 * 64);               // forward_knot_body's progress words (its rowbuf is ev)
            if (t == 0) { w[0] = 0u; w[2] = 0u; w[3] = 0u; w[4] = 0u; w[5] = st0; *verdict = 0u; }
            if (pst && t == 0) pst[wg == 0 ? 0 : 8] = (long long)wall_clock64();   // (wave 0 at the early barrier)
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
            if (pst && t == 0) pst[wg == 0 ? 1 : 9] = (long long)wall_clock64();   // (and out of it)
            if constexpr (FR) {
                bad = ((lds_vuptr)w)[5] != 0u;                       // (an LDS read by type)
                if (!bad && wg == 0 && t == 0) {                     // (the tag is formed where it is used: here by the leader's thread 0 alone, by everybody else behind the forward map)
                    unsigned tv = tag_v;
                    asm volatile("" : "+v"(tv));
                    tag = tv + 1u;
                    if (tag >= (1u << 28)) tag = 1u;
                }
            }
            else bad = *(volatile unsigned *)(w + 5) != 0u;
            if (!bad && wg == 0 && t == 0) __hip_atomic_store(flag, (tag << 4) | (my_xcc ? my_xcc : 15u), FRX_RLX_AGENT);
            return bad;
        };
        long long *est = nullptr;
        if (stp() && k == 0 && (wg == 0 || wg == wg_last)) est = stp() + (wg == 0 ? 50 : 60);
        long long *const fst = (stp() && k == 0 && wg == 0) ? stp() + 32 : nullptr;
        if constexpr (FR) {
            // the second trip: the loads the body would make from the index tables (KnotPre: its own expressions with the record's integers), wave 0's tau in front of them
            const int t2 = t - 64;                                   // index among the axis waves
            double tau = 0.0, r_bs[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
            asm volatile("" : "+v"(tau));                            // (the zero is written here, in front of the load: written behind it on the axis waves' path it would wait for every load of theirs)
            int r_pc = 0, r_piv = 1, r_wnv = 1, r_wvb = 0, r_wxb = 0;
            long long f_iss = 0;
            if (wave == 0) {
                if (fst) { asm volatile("" :: "v"(call.x + fr.x0 + lane), "v"(fr.nT)); f_iss = (long long)wall_clock64(); }
                if (lane < fr.nT) tau = call.x[fr.x0 + lane];
            }
            if (t < fr.N) { r_pc = l_pc[fr.p0 + t]; r_piv = l_piv[fr.p0 + t]; }
            const int wq = t2 >= 0 ? (t2 >> 1) : fr.N;               // waypoint wq is the axis waves' pair t2 >> 1
            if (wq < fr.N - 1) { const int gw = fr.wbase + wq; r_wnv = l_wnv[gw]; r_wvb = l_wvb[gw]; r_wxb = l_wxb[gw]; }
            if (t2 >= 0 && t2 < 3) {
                const gptr<const double> hd = l_head + c * 9, tl = l_tail + c * 9;     // (the candidate's base in scalar arithmetic)
#pragma unroll
                for (int q = 0; q < 3; q++) { r_bs[q] = hd[3 * q + t2]; r_bs[3 + q] = tl[3 * q + t2]; }
            }
            if (wave == 0 && fst) { asm volatile("" :: "v"(tau)); const long long f_in = (long long)wall_clock64(); if (lane == 0) { fst[0] = f_iss; fst[1] = f_in; } }
            const KnotPre kpre{fr.p0, fr.N, fr.c0, fr.cN, fr.x0, fr.cv0, r_pc, r_piv, r_wnv, r_wvb, r_wxb, {r_bs[0], r_bs[1], r_bs[2], r_bs[3], r_bs[4], r_bs[5]}};
            const EvalEarlySync<decltype(early), CH, true, PRE> es{early, est, wg == 0, nullptr, fr.nT, fr.nx, fr.nvd, ld.soft, ld.c2, l_vrec + 3 * (size_t)fr.cv0, tau, pst};
            forward_knot_body<false, 64, 5, 0, true>(a.dp, call.x, a.T, a.C, ld.maxCN, ld.maxXb, ld.maxVb, 64, nullptr, nsteps, c, ev, ctl, true, &ro, &kpre, nullptr, &es);
            asm volatile("" : "+v"(tag_v));
            tag = tag_v + 1u;
            if (tag >= (1u << 28)) tag = 1u;
        } else {
        const EvalEarlySync<decltype(early), CH> es{early, est, wg == 0, fst, 0, 0, 0, 0, 0, nullptr, 0.0, pst};
        forward_knot_body<false, 64, 5, 0, true>(a.dp, call.x, a.T, a.C, a.maxCN, a.maxXb, a.maxVb, 64, nullptr, nsteps, c, ev, ctl, true, &ro, nullptr, nullptr, &es);
        }
        if (bad) {                                                   // an earlier launch's wait expired (see above): uniform over the workgroup
            if (wg == 0 && t == 0) call.f[k] = __builtin_nan("");
            return;
        }
        if constexpr (GF) {
            if (has_task && lane < nh2) { hS[2 * lane] = hv[0].x; hS[2 * lane + 1] = hv[0].y; }   // (two 8-byte halves: a wave's LDS starts at an odd double, pen_lds = 1509)
        } else
        if (has_task) {
#pragma unroll
            for (int u = 0; u < 4; u++) { const int i = lane + 64 * u; if (i < nh2) { hS[2 * i] = hv[u].x; hS[2 * i + 1] = hv[u].y; } }
            for (int i0 = lane + 4 * 64; i0 < nh2; i0 += 4 * 64) {
                double2 v[4];
#pragma unroll
                for (int u = 0; u < 4; u++) { const int i = i0 + 64 * u; v[u] = h2[i < nh2 ? i : nh2 - 1]; }
#pragma unroll
                for (int u = 0; u < 4; u++) { const int i = i0 + 64 * u; if (i < nh2) { hS[2 * i] = v[u].x; hS[2 * i + 1] = v[u].y; } }
            }
        }
    } else {
    if (wg == 0) { if (t == 0) { *verdict = 0u; __hip_atomic_store(flag, (tag << 4) | (my_xcc ? my_xcc : 15u), FRX_RLX_AGENT); } }
    else if (has_task) {   // corridor blocks of the wave's task: constant, in flight under the forward map
        if (k == 0 && wg == 1 && wave == 0 && lane == 0 && stp()) stp()[44] = (long long)wall_clock64();
        for (int i0 = lane; i0 < nh2; i0 += 4 * 64) {
            double2 v[4];
#pragma unroll
            for (int u = 0; u < 4; u++) { const int i = i0 + 64 * u; v[u] = h2[i < nh2 ? i : nh2 - 1]; }
#pragma unroll
            for (int u = 0; u < 4; u++) { const int i = i0 + 64 * u; if (i < nh2) { hS[2 * i] = v[u].x; hS[2 * i + 1] = v[u].y; } }
        }
    }
    forward_knot_body<false, 64, 5>(a.dp, call.x, a.T, a.C, a.maxCN, a.maxXb, a.maxVb, 64, nullptr, nsteps, c, ev, ctl, true, &ro);   // MODE 1 | 4: stages x and the polytopes itself, (C, T) into ctl only
    }
    if (wg != 0) {
        // every WAVE of a member is on its own from here (no workgroup barrier below): its samples out of the workgroup's (C, T) copy, its partials as granules
        if (!has_task) return;
        long long *const mst = (k == 0 && wg == 1 && wave == 0 && lane == 0) ? stp() : nullptr;
        if (mst) mst[46] = (long long)wall_clock64();
        // (CH) what the reduction and the granule stores read from the argument block, once, in front of the samples
        int m_lpp = GC::lpp;
        if constexpr (!GF) m_lpp = a.lpp;
        int m_t0 = task * g_ppw(), m_N = N;
        ll_u64 *m_ll = nullptr;
        if constexpr (!GF) m_ll = a.out20ll + (size_t)p0 * 40;
        if constexpr (GF) {
            m_N = as_uniform(m_N);
            gptr<ll_u64> q_ll = as_uniform(m_llv);
            asm volatile("" : "+s"(m_N), "+s"(q_ll));
            m_ll = (ll_u64 *)q_ll;
        } else
        if constexpr (CH) {
            m_N = as_uniform(m_N);
            gptr<ll_u64> q_ll = (gptr<ll_u64>)as_uniform(m_ll);
            asm volatile("" : "+s"(m_lpp), "+s"(m_t0), "+s"(m_N), "+s"(q_ll));
            m_ll = (ll_u64 *)q_ll;
        }
        const int pl = lane / m_lpp, jl = lane - pl * m_lpp;
        if constexpr (GF) {
            DevProblem mdp = a.dp;
#pragma unroll
            for (int i = 0; i < 4; i++) mdp.pc.chi[i] = m_chi[i];
            mdp.inv_kappa = m_invk; mdp.kappa = m_kappa;
            if (pl < npieces) penalty_lane_samples<true>(mdp, ctl + (size_t)(m_t0 + pl) * 19, hS + (size_t)pl * hstride, ctl[(m_t0 + pl) * 19 + 18], jl, m_lpp, GC::kmax, red + lane * 21);
        } else
        if constexpr (CH) {
            // the penalty weights too: each is read inside the branch of its violated constraint, a scalar trip in the middle of a lane's samples
            DevProblem mdp = a.dp;
            asm volatile("" : "+s"(mdp.pc.chi[0]), "+s"(mdp.pc.chi[1]), "+s"(mdp.pc.chi[2]), "+s"(mdp.pc.chi[3]));
            if (pl < npieces) penalty_lane_samples<true>(mdp, ctl + (size_t)(m_t0 + pl) * 19, hS + (size_t)pl * hstride, ctl[(m_t0 + pl) * 19 + 18], jl, m_lpp, a.Kmax, red + lane * 21);
        } else
        if (pl < npieces) penalty_lane_samples<true>(a.dp, ctl + (size_t)(m_t0 + pl) * 19, hS + (size_t)pl * hstride, ctl[(m_t0 + pl) * 19 + 18], jl, m_lpp, a.Kmax, red + lane * 21);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if (mst) mst[47] = (long long)wall_clock64();
        const unsigned gv = __hip_atomic_load(flag, FRX_RLX_AGENT);           // the leader's XCD, if it has arrived under this evaluation's tag (requested in front of the samples instead, the trip is worth 0.07 us: profiles/NOTES.md)
        if (mst) { asm volatile("" :: "v"(gv)); mst[69] = (long long)wall_clock64(); }   // (the word's value is in its register)
        const bool wt = my_xcc == 0u || (gv >> 4) != tag || (gv & 15u) != my_xcc;   // plain stores when the leader runs on this XCD (its L2 is the meeting point), write-through otherwise
        if constexpr (HO) penalty_reduce<true, true>(red, npieces, m_lpp, nullptr, lane, 64, wt, m_ll, tag, m_N, m_t0);
        else penalty_reduce<true>(red, npieces, m_lpp, nullptr, lane, 64, wt, a.out20ll + (size_t)gp0 * 40, tag);
        if (mst) mst[48] = (long long)wall_clock64();
        return;
    }
    // ---- leader ----
    if (stp() && k == 0 && t == 0) stp()[41] = (long long)wall_clock64();
    ro.o20ll = a.out20ll; ro.o20tag = tag; ro.status = a.status; ro.spin_ticks = call.timeout_ticks;
    const LineSearchTap tap{nullptr, nullptr, nullptr, nullptr, nullptr, 0u, nullptr, nullptr};
    // the tail (EvalTail): f and `done` leave from inside the adjoint; the diagnostic's stamps 64.. of cluster 0 go with it
    // (CH) what the adjoint reads behind its poll, loaded here - the leader idles at the poll - and held in scalar registers: EvalChain, and the tail's addresses
    EvalChain ch{0.0, 0.0, 0, 0, nullptr};
    double *t_f = call.f; unsigned *t_done = done, *t_sh = call.status_host;
    if constexpr (CH) {
        ch = EvalChain{a.dp.rho, a.dp.sumT, a.dp.soft, a.dp.c2, nullptr};
        gptr<double> q_g = (gptr<double>)call.g, q_f = (gptr<double>)t_f;
        gptr<unsigned> q_done = (gptr<unsigned>)t_done, q_sh = (gptr<unsigned>)t_sh;
        asm volatile("" : "+s"(ch.rho), "+s"(ch.sumT), "+s"(ch.soft), "+s"(ch.c2), "+s"(q_g), "+s"(q_f), "+s"(q_done), "+s"(q_sh));
        ch.g = (double *)q_g; t_f = (double *)q_f; t_done = (unsigned *)q_done; t_sh = (unsigned *)q_sh;
    }
    const EvalTail tl{verdict, t_f, t_done, tag, t_sh, k == 0 ? stp() : nullptr, TAIL};
    const EvalHandoff<HO, CH, ADJ> ho{k == 0 ? stp() : nullptr, ch};
    backward_knot_body<true, 64, 0, EvalTail, EvalHandoff<HO, CH, ADJ>>(a.dp, call.x, a.T, a.C, nullptr, call.f, call.g, a.maxCN, a.maxXb, a.maxVb, 64, nullptr, nsteps, tap, c, ev, ctl, &ro, &tl, &ho);
    if (stp() && k == 0 && t == 0) stp()[42] = (long long)wall_clock64();
    if constexpr (TAIL) {
        if (stp() && k == 0 && t == 0) stp()[43] = (long long)wall_clock64();
    } else {
    __syncthreads();
    if (t == 0) {
        const double fv = ev[36 * 64 + 9 * 65 + 2 * 64 + a.maxCN];  // `red[0]` of backward_knot_wsp64: the objective value (a resident caller's f does not go to global memory there)
        const unsigned code = __hip_atomic_load(a.status, FRX_RLX_AGENT);
        const bool bad = code != 0u;
        if (tl.st) { asm volatile("" :: "v"(code)); tl.st[67] = (long long)wall_clock64(); }
        call.f[c] = bad ? __builtin_nan("") : fv;
        if (bad && call.status_host) __hip_atomic_store(call.status_host, code, FRX_RLX_SYS);
        __hip_atomic_store(done, tag, FRX_RLX_AGENT);
        if (tl.st) { const long long e = (long long)wall_clock64(); tl.st[68] = e; tl.st[43] = e; }
    }
    }
}

} // namespace frx
