// TEST INFRASTRUCTURE: a stand-alone host program around fast-racing_amd/csrc/frx_launch_forms.hpp, meant for a sanitizer build (tests/test_eval_adjoint_cpu.py compiles it with
// the address and undefined-behaviour sanitizers and runs it).  It enumerates the decision of the one-launch evaluation's adjoint switch (FRX_EVAL_ADJOINT, EvalSwitches::old_adjoint)
// over all nine switches and both inputs of eval_cluster_form: the rule written out once more, what the switch may NOT move, and the list of forms whose LDS limit is raised.
// Exit status 0 and no sanitizer report is the result.
#include <cstdio>
#include <memory>

#include "../../fast-racing_amd/csrc/frx_launch_forms.hpp"

using namespace frx;

int main() {
    int bad = 0, n = 0, with_adjoint = 0, taken = 0;
    for (int sw = 0; sw < 512; sw++) {
        const bool A = sw & 1, E = sw & 2, T = sw & 4, H = sw & 8, C = sw & 16, G = sw & 32, OF = sw & 64, OP = sw & 128, OA = sw & 256;
        EvalSwitches s{A, E, T, H, C, G};
        s.old_front = OF; s.old_prelude = OP; s.old_adjoint = OA;
        EvalSwitches s_def = s;
        s_def.old_adjoint = false;
        std::unique_ptr<EvalClusterForm[]> raised(new EvalClusterForm[4]);        // on the heap at its exact size: a form written past its end is reported
        const int nr = eval_cluster_raised_forms(s, raised.get());
        bad += nr < 1 || nr > 4;
        for (int k = 0; k < 4; k++) {
            const bool geom_class = k & 1, stamped = k & 2;
            EvalClusterForm f, d;
            const bool ok = eval_cluster_form(s, geom_class, stamped, true, f);
            bad += !ok || !eval_cluster_form(s_def, geom_class, stamped, true, d);
            // the rule, written out: an adjoint to take or to leave exists where the two-trip front (argument pointer, early durations, FRX_EVAL_FRONT not 0), the
            // value-major hand-off (which needs the inline tail) and the shortened prelude (FRX_EVAL_PRELUDE not 0) are all on; there the switch shows, inverted,
            // and nowhere else
            const bool has = A && E && !OF && (H && A && T) && !OP;
            bad += eval_form_has_adjoint(f) != has;
            bad += f.old_adjoint != (OA && has);
            bad += d.old_adjoint;                                                  // unset: the operands in front of the poll wherever that form exists
            // the switch moves nothing else
            EvalClusterForm g = f;
            g.old_adjoint = d.old_adjoint;
            bad += !(g == d);
            // and two forms that differ in it alone are two forms
            bad += (f == d) != (f.old_adjoint == d.old_adjoint);
            // the form a launch takes has had its limit raised
            int at = -1;
            for (int i = 0; i < nr; i++) if (raised[i] == f) at = i;
            bad += at < 0;
            // without a device block only the by-value form launches, and it never has the switch
            EvalClusterForm f0;
            bad += eval_cluster_form(s, geom_class, stamped, false, f0) != !f.argp || !(f0 == f);
            bad += !f.argp && f.old_adjoint;
            with_adjoint += has;
            taken += has && !f.old_adjoint;
            n++;
        }
    }
    // forms and switches written with the members that were there are the default ones in all three inverted flags
    const EvalClusterForm six{true, true, true, true, true, true};
    const EvalClusterForm eight{true, true, true, true, true, true, false, false};
    const EvalSwitches s8{true, true, true, true, true, true, false, false};
    bad += six.old_front || six.old_prelude || six.old_adjoint || !eval_form_has_adjoint(six);
    bad += eight.old_adjoint || !(eight == six) || s8.old_adjoint;
    n++;
    std::printf("%d decisions enumerated, %d with an adjoint to choose, %d of them take the operands in front of the poll, %d disagreements\n", n, with_adjoint, taken, bad);
    return bad ? 1 : 0;
}
