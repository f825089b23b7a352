// TEST INFRASTRUCTURE: a stand-alone host program around fast-racing_amd/csrc/frx_launch_forms.hpp, meant for a sanitizer build (make launch_forms_san).
// It runs the enumerations of tests/test_launch_forms_cpu.py in C++: every decision over all of its inputs, against the ladder of tests the launchers carried
// before the header existed, written out here once more.  Exit status 0 and no sanitizer report is the result.
#include <cstdio>
#include <memory>

#include "../../fast-racing_amd/csrc/frx_launch_forms.hpp"

using namespace frx;

// the ladder launch_eval_cluster had, rung by rung (the by-pointer rungs asked for the device block; the enumeration gives it)
static EvalClusterForm ladder(bool A, bool E, bool T, bool H, bool C, bool G, bool geom_class, bool stamped) {
    const bool handoff = H && A && T, chain = C && handoff, geom_on = G && handoff && E;
    if (geom_on && geom_class) {
        if (chain && !stamped) return {true, true, true, true, true, true};
        return {true, true, true, true, false, true};
    }
    if (chain && !stamped) return {true, E, true, true, true, false};
    if (handoff) return {true, E, true, true, false, false};
    if (A) {
        if (E && !T) return {true, true, false, false, false, false};
        return {true, E, true, false, false, false};
    }
    return {false, E, true, false, false, false};
}

// launch_penalty's tests in their order
static PenaltyForm penalty_ladder(bool lds_pen2, int lpp, int forced, char tp) {
    const bool lat = forced != 2, two_phase = tp != '0';
    if (lat && lds_pen2 && tp == '5') return PEN_LAT2_R5;
    if (lat && two_phase && lds_pen2) return lpp == 17 ? PEN_LAT2_17 : lpp == 49 ? PEN_LAT2_49 : PEN_LAT2_0;
    return lat ? PEN_LAT : PEN_THR;
}

// launch_eval's tests in their order
static EvalRoute route_ladder(bool backward, bool tap, bool cand_active, bool stamps, bool fused, bool fused_stamps, int solo, int B, int lo, int hi, bool lds_solo, bool knot) {
    const bool solo_ok = backward && lds_solo && knot && (!stamps || solo == 2);
    if (solo_ok && solo == 2) return EVAL_SOLO;
    if (backward && fused && knot && !tap && !cand_active && (!stamps || fused_stamps)) return EVAL_CLUSTER;
    if (solo_ok && solo == 1 && B >= lo && B <= hi) return EVAL_SOLO;
    return EVAL_STAGES;
}

int main() {
    int bad = 0, n = 0;
    for (int sw = 0; sw < 64; sw++) {
        const bool A = sw & 1, E = sw & 2, T = sw & 4, H = sw & 8, C = sw & 16, G = sw & 32;
        const EvalSwitches s{A, E, T, H, C, G};
        // the list on the heap at its exact size, so that a form written past its end is reported
        std::unique_ptr<EvalClusterForm[]> raised(new EvalClusterForm[4]);
        const int nr = eval_cluster_raised_forms(s, raised.get());
        bad += nr < 1 || nr > 4;
        int reached = 0;
        for (int k = 0; k < 4; k++) {
            const bool geom_class = k & 1, stamped = k & 2;
            EvalClusterForm f;
            const bool ok = eval_cluster_form(s, geom_class, stamped, true, f);
            bad += !ok || !(f == ladder(A, E, T, H, C, G, geom_class, stamped));
            EvalClusterForm f0;
            bad += eval_cluster_form(s, geom_class, stamped, false, f0) != !f.argp || !(f0 == f);   // no device block: only the by-value form launches
            int at = -1;
            for (int i = 0; i < nr; i++) if (raised[i] == f) at = i;
            bad += at < 0;                                                  // every form a launch can take has had its limit raised
            if (at >= 0) reached |= 1 << at;
            n++;
        }
        bad += reached != (1 << nr) - 1;                                    // and nothing else has
    }
    const char tps[4] = {0, '0', '1', '5'};
    for (int p2 = 0; p2 < 2; p2++) for (int lpp : {17, 49, 33}) for (int forced = 0; forced < 3; forced++) for (char tp : tps) {
        const PenaltyForm f = penalty_form(p2 != 0, lpp, forced, tp);
        bad += f != penalty_ladder(p2 != 0, lpp, forced, tp);
        bad += penalty_form_code(f) != (forced == 2 ? 0 : (p2 && tp != '0') ? 2 : 1);       // (frx_debug_penalty_kernel's own rule)
        n++;
    }
    for (int b = 0; b < 256; b++) for (int solo = 0; solo < 3; solo++) for (int B : {383, 384, 512, 513}) {
        const bool v[8] = {(b & 1) != 0, (b & 2) != 0, (b & 4) != 0, (b & 8) != 0, (b & 16) != 0, (b & 32) != 0, (b & 64) != 0, (b & 128) != 0};
        bad += eval_route(v[0], v[1], v[2], v[3], v[4], v[5], solo, B, 384, 512, v[6], v[7]) != route_ladder(v[0], v[1], v[2], v[3], v[4], v[5], solo, B, 384, 512, v[6], v[7]);
        n++;
    }
    bad += pen_wave_doubles(3, 8) != 1509 || pen_wave_doubles(7, 8) != 7 * 19 + 7 * 36 + 1344 || pen_wave_doubles(1, 14) != 19 + 60 + 1344;
    bad += pen_wg_bytes(15, 8, 4, 21) != (size_t)8 * (15 * 19 + 15 * 36 + 256 * 21) || pen_wg_bytes(15, 8, 4, 11) != (size_t)8 * (15 * 19 + 15 * 36 + 256 * 11);
    n += 5;
    {   // the grow-only table with a setter that only counts: large, small, large again, larger; a failed call; another function and another device
        LdsLimits limits;
        int calls = 0, fn_a = 0, fn_b = 0;
        auto set = [&](const void *, size_t) { calls++; return 0; };
        bad += limits.raise(0, &fn_a, 98304, set) != 0 || calls != 1;
        bad += limits.raise(0, &fn_a, 4096, set) != 0 || calls != 1;
        bad += limits.raise(0, &fn_a, 98304, set) != 0 || calls != 1;
        bad += limits.raise(0, &fn_a, 0, set) != 0 || calls != 1;
        bad += limits.raise(0, &fn_a, 163840, [&](const void *, size_t) { return 7; }) != 7;      // refused: nothing is held for it
        bad += limits.raise(0, &fn_a, 163840, set) != 0 || calls != 2;
        bad += limits.raise(0, &fn_b, 4096, set) != 0 || calls != 3;
        bad += limits.raise(1, &fn_a, 4096, set) != 0 || calls != 4;
        n += 8;
    }
    std::printf("%d decisions enumerated, %d disagreements with the ladders\n", n, bad);
    return bad ? 1 : 0;
}
