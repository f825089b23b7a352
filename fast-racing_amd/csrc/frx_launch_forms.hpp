// Which kernel form a launch takes, as pure functions of integers and bools, and the grow-only table of the kernels' LDS limits: shared by the launchers
// (frx_device*.hip), the diagnostics that report a form (frx_api.cpp) and the CPU-side enumeration of every decision (tests/test_launch_forms_cpu.py).  Plain C++,
// no HIP, no environment: the callers read the switches and make the HIP calls.
#pragma once
#include <cstddef>
#include <map>
#include <utility>

namespace frx {

// ---- LDS of the penalty integrator: piece records | corridor blocks of Kmax + 1 records | the lanes' partials ----
// doubles per WAVE (penalty_body with a 64-lane group: the resident round kernel, the one-launch evaluation)
constexpr int pen_wave_doubles(int ppw, int Kmax) { return ppw * 19 + ppw * (Kmax + 1) * 4 + 64 * 21; }
// bytes per WORKGROUP of `waves` waves (stage kernels): 21 doubles per lane in the one-phase forms, 11 in the two-phase ones
constexpr size_t pen_wg_bytes(int ppg, int Kmax, int waves, int doubles_per_lane) {
    return sizeof(double) * ((size_t)ppg * 19 + (size_t)ppg * (Kmax + 1) * 4 + (size_t)64 * waves * doubles_per_lane);
}

constexpr size_t LDS_PER_CU = (size_t)160 * 1024;                 // what a workgroup can have (gfx950)

// ---- LDS of the knot kernels: each is the sum of what the kernel's carve-up takes from its one dynamic array (frx_kernels.hpp names the function at the carve-up) ----
constexpr int knot_threads(int maxN) { return 64 * ((maxN + 63) / 64); }                       // rows of the knot system's buffers: maxN rounded up to whole waves
constexpr int pcr_steps(int maxN) { int n = 0; for (int s = 1; s < maxN - 1; s <<= 1) n++; return n; }   // ceil(log2(maxN - 1)), 0 up to two pieces
// forward_knot_body: row buffer 36 nt | KP KV KA 3 x 3 (nt + 1) | Tf nt | Tc maxCN | xs maxXb | vs maxVb | the saved multipliers (8 steps + 5) nt
constexpr size_t knot_fwd_lds_bytes(int knot_threads, int maxCN, int maxXb, int maxVb, int pcr_steps) {
    const size_t nt = knot_threads;
    return sizeof(double) * (36 * nt + 9 * (nt + 1) + nt + maxCN + maxXb + maxVb + (size_t)(pcr_steps * 8 + 5) * nt);
}
// the backward_knot bodies: as above with gT nt beside Tf, gCo for Tc, the cross-wave partials red 2 x 4 + 2 and the search direction dsv maxXb behind the multipliers
constexpr size_t knot_bwd_lds_bytes(int knot_threads, int maxCN, int maxXb, int maxVb, int pcr_steps) {
    const size_t nt = knot_threads;
    return sizeof(double) * (36 * nt + 9 * (nt + 1) + 2 * nt + maxCN + 2 * 4 + 2 + 2 * maxXb + maxVb + (size_t)(pcr_steps * 8 + 5) * nt);
}
// (the banded-LU pair's sizes stand beside the band width they depend on: banded_fwd_lds_bytes / banded_bwd_lds_bytes, frx_device.hpp)

// ---- what a handle's geometry admits (frx_problem_create turns a refusal into its message) ----
enum GeomRefusal { GEOM_FITS, GEOM_KNOT_CAPACITY, GEOM_PENALTY_CAPACITY };
struct GeomVerdict { GeomRefusal refusal; bool banded_ok; };
// the knot system of the largest candidate must fit one workgroup, the penalty workgroup one CU; the banded-LU cross-check kernels need the whole band in LDS and
// are "unavailable" instead of failing create
constexpr GeomVerdict geometry_verdict(int knot_threads, size_t lds_kbwd, size_t lds_fwd, size_t lds_bwd, size_t lds_pen) {
    return {knot_threads > 256 || lds_kbwd > LDS_PER_CU ? GEOM_KNOT_CAPACITY : lds_pen > LDS_PER_CU ? GEOM_PENALTY_CAPACITY : GEOM_FITS,
            !(lds_bwd > LDS_PER_CU || lds_fwd > LDS_PER_CU)};
}

// ---- stage kernel k_penalty: waves per workgroup and the whole pieces they own ----
// A workgroup of W waves owns floor(64 W / lpp) whole pieces; W in 1..4 for the best lane utilisation (the fewest waves among equals) - kappa = 16: 51/64 lanes with
// one wave, 255/256 with four; stock kappa = 48: 49/64 and 245/256.  Measured (profiles/r03_penalty_waves_per_workgroup.jsonl, kappa = 16): 1024 candidates
// 40.3 -> 35.9 us, 4096 candidates 153 -> 132 us (kappa = 48, 1024 candidates: 116 -> 95 us); but a launch that fits the chip's SIMDs in one go is ONE wave's latency,
// and there one-wave workgroups (no barrier, twice the CUs in use) win: 4.79 against 5.17 us at the headline batch.  forced_waves: FRX_PENALTY_WAVES as a number,
// 1..4 overrides, anything else does not.
struct PenaltyWaves { int pen_w, ppg; };
inline PenaltyWaves penalty_waves(int lpp, int Kmax, int P, int simds, int forced_waves) {
    const int ppw = 64 / lpp;
    int best_w = 1; double best_u = 0.0;
    for (int w = 1; w <= 4; w++) {
        const double u = (double)((64 * w) / lpp * lpp) / (64.0 * w);
        if (u > best_u + 1e-9) { best_u = u; best_w = w; }
    }
    if ((P + ppw - 1) / ppw <= simds) best_w = 1;
    if (forced_waves >= 1 && forced_waves <= 4) best_w = forced_waves;
    //  W is chosen for lane utilisation, but the workgroup's LDS grows with it (ppg corridor blocks of Kmax + 1 records): step W down
    // until the block fits the CU - a corridor with many half-spaces runs on fewer waves instead of failing create
    while (best_w > 1 && pen_wg_bytes((64 * best_w) / lpp, Kmax, best_w, 21) > LDS_PER_CU) best_w--;
    return {best_w, (64 * best_w) / lpp};
}

// ---- which handles take the one-launch and the solo evaluation ----
// One launch per evaluation when every cluster of the batch gets its CUs at once (G workgroups per candidate, 0 = the geometry does not apply).  fused_char: first
// character of FRX_EVAL_FUSED, 0 when unset.   ranks of one node that SHARE a device (more local ranks than devices): their grids would compete for the CUs
// a cluster's leader assumes - off unless asked for (FRX_EVAL_FUSED=1); a lone process, or one rank per device, takes the form
constexpr bool eval_cluster_admitted(int G, int B, int cus, char fused_char, int local_ranks, int ndev) {
    return G && (long long)B * G <= cus && fused_char != '0' && !(local_ranks > ndev && fused_char != '1');
}
// The solo form: from the batch size on at which the stage launches' ramps and stage-buffer trips outweigh a lone workgroup's five penalty passes - measured,
// profiles/NOTES.md round 6.  solo_char: first character of FRX_EVAL_SOLO ('0' never, '1' always), 0 when unset; min_B / max_B: FRX_EVAL_SOLO_MIN_B / _MAX_B as
// numbers, > 0 moves the threshold.  eval_solo as frx_problem holds it: 0 never, 1 inside [min_B, max_B], 2 always.
struct SoloChoice { int eval_solo, min_B, max_B; };
constexpr SoloChoice eval_solo_choice(bool lds_solo, char solo_char, int min_B, int max_B) {
    return {solo_char == '0' ? 0 : solo_char == '1' && lds_solo ? 2 : lds_solo ? 1 : 0, min_B > 0 ? min_B : 384, max_B > 0 ? max_B : 512};
}

// ---- the dynamic-LDS limit of every kernel (raise_lds_limit, frx_device.hip) ----
// What is held per (device, function), and the rule: the limit only grows.  set(fn, bytes) makes the call (0 = done) and is only asked for a need above what is
// held; a need already held, or none at all, is no call.  A failed call leaves the table as it was.
class LdsLimits {
    std::map<std::pair<int, const void *>, size_t> held_;
public:
    template <class Set> int raise(int dev, const void *fn, size_t bytes, Set &&set) {
        if (!bytes) return 0;
        size_t &held = held_[{dev, fn}];
        if (bytes <= held) return 0;
        const int e = set(fn, bytes);
        if (!e) held = bytes;
        return e;
    }
};

// ---- k_eval_cluster<ARGP, ET, TAIL, HO, CH, GEO, FR, PRE, ADJ> ----
// geo: the geometry class EvalGeomK16.  old_front (FR = false; only with argp and et - false in every other form): the front that walks the offset tables, FRX_EVAL_FRONT=0;
// an inverted flag, so that a form written with the six members in front of it is the default one.  old_prelude (PRE = false; only where the shortened prelude of the
// forward map exists - the two-trip front with the value-major hand-off - and false in every other form): the prelude before, FRX_EVAL_PRELUDE=0; inverted likewise.
// old_adjoint (ADJ = false; only where the shortened prelude is on - and false in every other form): the leader's adjoint as it was, FRX_EVAL_ADJOINT=0; inverted likewise
struct EvalClusterForm { bool argp, et, tail, ho, ch, geo; bool old_front = false; bool old_prelude = false; bool old_adjoint = false; };
inline bool operator==(const EvalClusterForm &a, const EvalClusterForm &b) {
    return a.argp == b.argp && a.et == b.et && a.tail == b.tail && a.ho == b.ho && a.ch == b.ch && a.geo == b.geo && a.old_front == b.old_front && a.old_prelude == b.old_prelude &&
           a.old_adjoint == b.old_adjoint;
}
// has this form a shortened prelude to take or to leave?  (the two-trip front - argp, et, not old_front - and the value-major hand-off)
constexpr bool eval_form_has_prelude(const EvalClusterForm &f) { return f.argp && f.et && !f.old_front && f.ho; }
// has this form the adjoint's operands in front of the poll to take or to leave?  (the two-trip front, the value-major hand-off and the shortened prelude all on)
constexpr bool eval_form_has_adjoint(const EvalClusterForm &f) { return eval_form_has_prelude(f) && !f.old_prelude; }
// the six FRX_EVAL_* switches as set (true unless the variable begins with '0'); a switch only counts with the ones in front of it at their defaults.
// old_front: FRX_EVAL_FRONT begins with '0' (inverted: unset is false) - it shows in every form with the argument pointer and early durations, and selects no other form.
// old_prelude: FRX_EVAL_PRELUDE begins with '0' (inverted likewise) - it shows in every form with the two-trip front and the value-major hand-off, and selects no other form.
// old_adjoint: FRX_EVAL_ADJOINT begins with '0' (inverted likewise) - it shows in every form that has the shortened prelude on, and selects no other form
struct EvalSwitches {
    bool argptr, early_t, tail, handoff, chain, geom; bool old_front = false; bool old_prelude = false; bool old_adjoint = false;
    constexpr bool handoff_on() const { return handoff && argptr && tail; }
    constexpr bool chain_on() const { return chain && handoff_on(); }
    constexpr bool geom_on() const { return geom && handoff_on() && early_t; }
};
// The form a launch takes.  geom_class: the handle has the one-launch form and its geometry equals the class's integers; stamped: the argument block carries the
// stamps pointer (a diagnostic's evaluation - the production chain has no stamp code).  FRX_EVAL_TAIL=0 only shows with the argument pointer and early durations.
// Returns false when the form takes its arguments by pointer and there is no device block.
inline bool eval_cluster_form(const EvalSwitches &s, bool geom_class, bool stamped, bool have_dev_args, EvalClusterForm &f) {
    const bool chained = s.chain_on() && !stamped;
    if (s.geom_on() && geom_class) f = {true, true, true, true, chained, true};
    else if (s.handoff_on()) f = {true, s.early_t, true, true, chained, false};
    else if (s.argptr) f = {true, s.early_t, !(s.early_t && !s.tail), false, false, false};
    else f = {false, s.early_t, true, false, false, false};
    f.old_front = s.old_front && f.argp && f.et;
    f.old_prelude = s.old_prelude && eval_form_has_prelude(f);
    f.old_adjoint = s.old_adjoint && eval_form_has_adjoint(f);
    return !f.argp || have_dev_args;
}
// The forms whose dynamic-LDS limit a process raises: every form eval_cluster_form can give under these switches.  Returns their number: at most 4, one per
// value of (geom_class, stamped); old_front, old_prelude and old_adjoint are per-process switches, not inputs - an input added to eval_cluster_form is one more loop here and doubles the bound.
inline int eval_cluster_raised_forms(const EvalSwitches &s, EvalClusterForm out[4]) {
    int n = 0;
    for (int geom_class = 0; geom_class <= (s.geom_on() ? 1 : 0); geom_class++)
        for (int stamped = 0; stamped <= (s.chain_on() ? 1 : 0); stamped++) (void)eval_cluster_form(s, geom_class, stamped, true, out[n++]);
    return n;
}

// ---- the stage launch of the penalty integral ----
enum PenaltyForm { PEN_THR, PEN_LAT, PEN_LAT2_17, PEN_LAT2_49, PEN_LAT2_0, PEN_LAT2_R5 };
// the two-phase instantiation of a geometry: the two boundary resolutions kappa = 16 / 48 have their own
constexpr PenaltyForm penalty_lat2_form(int lpp) { return lpp == 17 ? PEN_LAT2_17 : lpp == 49 ? PEN_LAT2_49 : PEN_LAT2_0; }
// forced: FRX_PENALTY_FORM unset 0, 'l..' 1, anything else 2 (the throughput form); twophase_char: first character of FRX_PENALTY_TWOPHASE, 0 when unset
// ('0': the one-phase launch, '5': the round-5 form, A/B)
constexpr PenaltyForm penalty_form(bool lds_pen2, int lpp, int forced, char twophase_char) {
    return forced == 2 ? PEN_THR : !lds_pen2 || twophase_char == '0' ? PEN_LAT : twophase_char == '5' ? PEN_LAT2_R5 : penalty_lat2_form(lpp);
}
constexpr int penalty_form_code(PenaltyForm f) { return f == PEN_THR ? 0 : f == PEN_LAT ? 1 : 2; }   // (frx_debug_penalty_kernel)

// ---- the route of an evaluation ----
enum EvalRoute { EVAL_CLUSTER, EVAL_SOLO, EVAL_STAGES };
// A plain evaluation of a batch the chip holds at once: ONE launch of clusters; batches beyond their reach (and the optimiser's rounds there): one workgroup per
// candidate; else the three stage kernels.  eval_solo: 0 never, 1 inside [solo_min_B, solo_max_B], 2 forced (in front of the clusters, and with the cycle stamps).
constexpr EvalRoute eval_route(bool backward, bool tap, bool cand_active, bool stamps, bool eval_fused, bool eval_fused_stamps, int eval_solo, int B, int solo_min_B,
                               int solo_max_B, bool lds_solo, bool knot_solver) {
    const bool solo_ok = backward && lds_solo && knot_solver && (!stamps || eval_solo == 2);
    return solo_ok && eval_solo == 2 ? EVAL_SOLO
         : backward && eval_fused && knot_solver && !tap && !cand_active && (!stamps || eval_fused_stamps) ? EVAL_CLUSTER
         : solo_ok && eval_solo == 1 && B >= solo_min_B && B <= solo_max_B ? EVAL_SOLO : EVAL_STAGES;
}

} // namespace frx
