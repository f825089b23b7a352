"""The device forms of the MINCO map (tau, xi) -> (T, q) -> c and of its adjoint against an EXACT solve (tests/minco_reference.py: numpy.longdouble, pivoted LU,
iterative refinement, its own residual asserted <= 1e-15 max|b| inside every solve) at uneven durations: one candidate per duration family (all inside [0.02, 5]:
even, geometric ramp, log-uniform, alternating 0.02 / 5, one short piece first / last / in the middle of pieces of 1.0, one long piece among short ones), one handle
per N in {1, 2, 3, 5, 9, 33, 64, 65, 128}.

Route taken for f = J + rho sum T ("jerk"): every penalty weight ZERO (penalty_pvtb = (0, 0, 0, 0) through frx.Problem's overrides; it is accepted and gives no NaN at
these speeds), so the penalty integrator runs and adds nothing, and the adjoint's only input is dJ/dc.  That input has no component along the knot derivatives (the
spline minimises J over them): the adjoint's knot solve gets a zero right-hand side.  A second objective ("speed": minco_reference.SPEED_PENALTY, the reference's
speed term alone at vel_max = 1 and weight 1, restated exactly in long double) gives it one.  tau comes from the family's durations by backwardT, xi is the handle's
own initial guess.

Per candidate, against exact: T at 1e-13; c0 of every piece after the first = the exact waypoint to 1e-13 of the position scale; C raw at 1e-7 of max|C| (knot form) /
1e-9 (banded LU); C duration-normalised at 1e-11 (global) and 1e-9 (per piece shape); f at 1e-9; the tau block and the xi block of the gradient EACH at 1e-9 of its own
largest exact entry, with no |f| floor (tests/test_minco_exact_cpu.py asserts that no block of these cases is small against f).

Forms, each shown to be the one that ran by the handle's queries: the three stage launches of the knot form, the banded-LU pair, the one-launch evaluation where it
applies (<= 64 pieces), the solo launch forced where it applies.  That the one-launch and three-launch forms agree with each other is tests/test_gpu_parity.py's.
Measured: every knot form holds every tolerance at every case; the banded-LU pair misses a few figures (KNOWN_LOSSES below: expected failures, one figure at a time).
Run with -s for the measured figures (DESIGN.md records them)."""
import numpy as np
import pytest

import minco_reference as mr

pytestmark = pytest.mark.gpu

PER_EVAL_TOL = mr.PER_EVAL_TOL
KAPPA = 8
_exact = {}                                                                # (N, family, layer, objective) -> mr.Exact: the long-double solves, once per module


def exact(sc, N, family, layer, objective, cand, tau, xi):
    key = (N, family, layer, objective)
    if key not in _exact:
        pen = None if objective == "jerk" else dict(kappa=KAPPA, **mr.SPEED_PENALTY)
        other = _exact.get((N, family, layer, "speed" if objective == "jerk" else "jerk"))
        _exact[key] = mr.Exact(cand, layer, tau, xi, sc.ZHANGJIAJIE["rho"], mr.total_time(N), pen=pen, forward_of=other)
    ex = _exact[key]
    assert np.array_equal(ex.tau, tau) and np.array_equal(ex.xi, xi)
    return ex


def handle(frx, sc, N, layer, objective, families):
    cands = [mr.candidates(sc, N)[f] for f in families]
    over = dict(penalty_pvtb=(0.0, 0.0, 0.0, 0.0)) if objective == "jerk" else mr.speed_penalty_overrides()
    prob = frx.Problem(cands, sc.ZHANGJIAJIE, qd_intervals=KAPPA, **over, **mr.layer_overrides(layer, mr.total_time(N)))
    assert prob.B == len(families) and prob.P == len(families) * N
    x = prob.initial_guess()
    refs = []
    for b, f in enumerate(families):
        nt = int(prob.dim_t[b]); lo = int(prob.x_off[b]); hi = int(prob.x_off[b + 1])
        tau = mr.family_tau(N, f, layer)
        assert tau.size == nt == (N if layer == "soft_c2" else N - 1)
        x[lo:lo + nt] = tau
        refs.append(exact(sc, N, f, layer, objective, cands[b], tau, x[lo + nt:hi].copy()))
    return prob, x, refs


def check_forward(prob, x, refs, families, solver, tag, assert_coefficients=True):
    """[(family, metric, value)] of every figure of the forward map that misses its tolerance."""
    T, Cf = prob.forward(x)
    N = prob.P // prob.B
    missed = []
    for b, (ex, fam) in enumerate(zip(refs, families)):
        sl = slice(int(prob.piece_off[b]), int(prob.piece_off[b + 1]))
        Tb, Cb = T[sl], Cf[6 * sl.start:6 * sl.stop]
        eT = mr.rel(Tb, ex.T)
        eq = float(np.abs(Cb[6::6].astype(mr.LD) - ex.q).max() / ex.pos_scale) if N > 1 else 0.0
        raw = mr.rel(Cb, ex.C)
        eg, ep = mr.coeff_err_normalised(Cb, ex.C, ex.T)
        print(f"{tag} N={N} {fam}: T {eT:.1e}  q {eq:.1e}  C raw {raw:.1e}  normalised {eg:.1e} / per piece {ep:.1e}")
        limits = [("T", eT, 1e-13), ("q", eq, 1e-13)]
        if assert_coefficients:
            limits += [("raw", raw, 1e-7 if solver == "knot_pcr" else PER_EVAL_TOL), ("normalised", eg, 1e-11), ("per piece", ep, PER_EVAL_TOL)]
        missed += [(fam, name, v) for name, v, lim in limits if not v < lim]
    return missed


def check_objective(prob, x, refs, families, tag, tol=PER_EVAL_TOL):
    """[(family, metric, value)] of f and of the two gradient blocks where they miss tol."""
    f, g = prob.objective(x)
    N = prob.P // prob.B
    missed = []
    for b, (ex, fam) in enumerate(zip(refs, families)):
        nt = int(prob.dim_t[b]); lo = int(prob.x_off[b]); hi = int(prob.x_off[b + 1])
        ef = float(abs(mr.LD(f[b]) - ex.f) / abs(ex.f))
        e_tau, e_xi = mr.block_err(g[lo:lo + nt], ex.g_tau), mr.block_err(g[lo + nt:hi], ex.g_xi)
        print(f"{tag} N={N} {fam}: f {ef:.1e}  g_tau {e_tau:.1e}  g_xi {e_xi:.1e}")
        missed += [(fam, name, v) for name, v in (("f", ef), ("g_tau", e_tau), ("g_xi", e_xi)) if not v <= tol]
    return missed


def run_form(prob, x, refs, families, form, tag, assert_coefficients=True, tol=PER_EVAL_TOL):
    """One form of the handle, behind the queries that show it is the one the next evaluation takes; returns the figures that miss."""
    N = prob.P // prob.B
    prob.set_solver("knot_pcr"); prob.set_eval_solo(0); prob.set_eval_fused(False)
    if form == "three":                                                      # three stage launches: k_forward_knot*, the penalty kernel, k_backward_knot*
        assert prob.eval_fused() == 0 and prob.eval_solo() == 0
        missed = check_forward(prob, x, refs, families, "knot_pcr", f"[{tag}, knot form, three launches]", assert_coefficients)
        missed += check_objective(prob, x, refs, families, f"[{tag}, knot form, three launches]", tol)
        if N > 64:                                                           # ... the only knot form beyond 64 pieces
            prob.set_eval_fused(True)
            assert prob.eval_fused() == 0 and not prob.solo_applies()
    elif form == "banded":                                                   # k_forward / k_backward
        prob.set_solver("banded_lu")
        assert prob.eval_fused() == 0 and prob.eval_solo() == 0
        missed = check_forward(prob, x, refs, families, "banded_lu", f"[{tag}, banded LU]", assert_coefficients)
        missed += check_objective(prob, x, refs, families, f"[{tag}, banded LU]", tol)
    elif form == "one":                                                      # k_eval_cluster
        prob.set_eval_fused(True)
        assert N <= 64 and prob.eval_fused() > 0 and prob.eval_solo() == 0, "the one-launch form applies to every small batch of <= 64 pieces"
        missed = check_objective(prob, x, refs, families, f"[{tag}, one launch of {prob.eval_fused()} workgroups]", tol)
    else:                                                                    # k_eval_solo, in front of the clusters
        assert N <= 64 and prob.solo_applies(), "the solo form applies to <= 64 pieces at 9 samples per piece"
        prob.set_eval_fused(True); prob.set_eval_solo(2)
        assert prob.eval_solo() >= 1
        missed = check_objective(prob, x, refs, families, f"[{tag}, solo launch]", tol)
    return missed


def forms_of(N, banded=True):
    return ["three"] + (["banded"] if banded else []) + (["one", "solo"] if N <= 64 else [])


# the jerk objective: the soft layer at every N, the fixed-time layers at N = 9 and 64; the speed objective: wherever there is a knot to solve for, the fixed-time layers at N = 9
STATES = [(N, "soft_c2", "jerk") for N in mr.SIZES] + [(N, layer, "jerk") for N in (9, 64) for layer in ("fixed_c2", "fixed_exp")] + \
         [(N, "soft_c2", "speed") for N in mr.SIZES if N > 1] + [(9, layer, "speed") for layer in ("fixed_c2", "fixed_exp")]
CASES = [(N, layer, objective, form) for N, layer, objective in STATES for form in forms_of(N)]

# Genuine losses inside the asserted duration range, as measured on an MI355X: (N, layer, objective, form) -> {(family, metric): measured}.  Every other figure of
# the case stands at its tolerance, and an entry here that no longer misses fails the test as well (the strictness of an expected failure, one figure at a time).
# All of them belong to the banded-LU cross-check kernels, i.e. to the reference's elimination order without pivoting in float64: the CPU oracle, which runs the same
# elimination, misses the same waypoint figures (to the last digit at N = 5, 9 and 33), while every knot form holds every tolerance.  There c0 is the outcome of the solve, not the
# waypoint itself, and a 5 s piece beside a 0.02 s piece costs it 1e-12 of the position scale; the long piece among short ones takes the duration-normalised
# coefficients to 1.3e-11 of the largest one ("Against an exact solve").
_BANDED_LOSSES = {(3, "soft_c2"): {("alternating", "q"): 1.4e-12, ("long_middle", "q"): 2.4e-13},
                  (5, "soft_c2"): {("alternating", "q"): 2.4e-12, ("long_middle", "normalised"): 1.2e-11},
                  (9, "soft_c2"): {("alternating", "q"): 1.3e-12, ("long_middle", "normalised"): 1.3e-11},
                  (33, "soft_c2"): {("alternating", "q"): 4.1e-13},
                  (9, "fixed_c2"): {("alternating", "q"): 9.9e-13},
                  (9, "fixed_exp"): {("alternating", "q"): 9.9e-13}}
KNOWN_LOSSES = {(N, layer, objective, "banded"): v for (N, layer), v in _BANDED_LOSSES.items() for objective in ("jerk", "speed")}


@pytest.mark.parametrize("N,layer,objective,form", CASES)
def test_form_against_exact_at_uneven_durations(frx, sc, N, layer, objective, form):
    families = list(mr.ASSERTED_FAMILIES)
    prob, x, refs = handle(frx, sc, N, layer, objective, families)
    missed = run_form(prob, x, refs, families, form, f"{layer} {objective}")
    prob.close()
    known = KNOWN_LOSSES.get((N, layer, objective, form), {})
    assert {(fam, name) for fam, name, _ in missed} == set(known), ([m for m in missed if m[:2] not in known], [k for k in known if k not in {m[:2] for m in missed}])


@pytest.mark.parametrize("N,objective,form", [(N, objective, form) for objective in ("jerk", "speed") for N in (3, 9, 64, 128) for form in forms_of(N, banded=False)])
def test_one_piece_a_thousand_times_shorter_than_its_neighbours(frx, sc, N, objective, form):
    """1e-3 among 1.0, soft layer, the knot form in its three-launch, one-launch and solo forms: T, f and both gradient blocks of the jerk objective hold the tolerances
    above.  The coefficients are printed and NOT asserted: the knot form's leave the 1e-11 / 1e-9 envelope at this duration ratio (the asserted contract is
    [0.02, 5]).  A functional that reads the coefficients inherits their error: the speed objective is printed too and held only to the project's end-to-end figure, 1e-6."""
    families = [mr.EXTREME_FAMILY]
    prob, x, refs = handle(frx, sc, N, "soft_c2", objective, families)
    missed = run_form(prob, x, refs, families, form, f"soft_c2 {objective}", assert_coefficients=False, tol=PER_EVAL_TOL if objective == "jerk" else 1e-6)
    prob.close()
    assert not missed, missed
