"""The scalars that cross the mailbox of the per-stage rounds - f, g.d, x.x, g.g and, after INIT / ADVANCE, gp.d - against an independent replay: candidate 0's
traced commands (FRX_TRACE) are applied open loop to the long-double model of the vector commands (dv_reference) with the CPU oracle as the objective, each
row with its own flags and step.  The scalars come from the LineSearchTap of three adjoint bodies (the stage form for <= 64 pieces, the general body above,
the solo launch) and, on banded LU, from k_lbfgs_post; until now they were only compared between two device paths.

The window ends with the 10th ADVANCE row: an open-loop replay is path sensitive - a replay whose directions were summed in another order drifted from the
solver's f by <= 3e-13 after 10 accepted steps, <= 3e-11 after 20, up to 9e-8 after 30 (CPU, five candidates) - and 1e-9 has to mean the kernels."""
import os

import numpy as np
import pytest

import dv_reference as ref
import dv_states as dvs
from dv_reference import DV_ADVANCE, DV_INIT

pytestmark = pytest.mark.gpu

KAPPA = 8
SHORT_FIRST = [(7, 12, 3, False), (4, 24, 6, True), (0, 32, 8, False)]
LONG_FIRST = SHORT_FIRST[::-1]
HUNDRED = [(3, 100, 25, False), (7, 12, 3, False), (4, 24, 6, True)]          # candidate 0 has 100 pieces: the general adjoint body

FORMS = [("stage", SHORT_FIRST), ("stage", LONG_FIRST), ("solo", SHORT_FIRST), ("solo", LONG_FIRST), ("stage", HUNDRED),
         ("banded_lu", SHORT_FIRST), ("banded_lu", LONG_FIRST), ("skip_inactive", SHORT_FIRST), ("skip_inactive", LONG_FIRST)]


def replay(frx, o, x0, rows, m=128, window=10):
    """Candidate 0's traced rows {flags, step, f, g.d, gp.d_new, x.x, g.g} applied open loop to the model from x0, the oracle `o` as the objective, through the
    `window`-th ADVANCE row; m = the planner's history length (frx_lbfgs_gcopter_params).  Returns (violations, worst error / tolerance per scalar, ADVANCE rows
    seen, rows used).  Tolerances: 1e-9 relative for f, x.x, g.g, gp.d; g.d by 1e-9 max(|g|inf, |f|) |d|_1 (the gradient parity the suite holds the evaluation
    to: g.d can legitimately be near zero)."""
    n = o.n
    geom, hs = frx.dv_layout(n)
    st = dvs.new_state(frx, [n], m, geom, hs, np.random.default_rng(0))
    lo, hi = int(st["xoff"][0]), int(st["xoff"][1])
    st["x"][lo:hi] = x0
    advances, have_d, worst, used = 0, False, {}, 0
    bad = []
    for i, (flags, step, f, dg, dginit, xx, gg) in enumerate(rows):
        fl = int(flags)
        cmd = np.zeros(1, frx.DV_COMMAND)
        cmd[0]["flags"] = fl; cmd[0]["step"] = step
        if fl & DV_ADVANCE:
            cmd[0]["slot"] = cmd[0]["newest"] = advances % m; cmd[0]["bound"] = min(advances + 1, m)
            advances += 1
        ref.apply(st, cmd)                                              # the vector part: direction and trial point
        have_d |= bool(fl & (DV_INIT | DV_ADVANCE))                     # (before the INIT row the device's d is whatever the allocation held)
        x, d = st["x"][lo:hi], st["d"][lo:hi]
        f_ref, g_ref = o.objective(x.copy())                            # the evaluation
        st["g"][lo:hi] = g_ref
        want = dict(f=(f, f_ref, 1e-9 * abs(f_ref)), xx=(xx, float(ref.ld_dot(x, x)[0]), None), gg=(gg, float(ref.ld_dot(g_ref, g_ref)[0]), None))
        if have_d:
            want["dg"] = (dg, float(ref.ld_dot(g_ref, d)[0]), 1e-9 * max(np.abs(g_ref).max(), abs(f_ref)) * np.abs(d).sum())
        if fl & (DV_INIT | DV_ADVANCE):
            want["dginit"] = (dginit, float(st["res"]["dginit"][0]), None)
        for k, (got, exp, tol) in want.items():
            tol = 1e-9 * abs(exp) if tol is None else tol
            err = abs(got - exp)
            worst[k] = max(worst.get(k, 0.0), err / tol if tol > 0 else (0.0 if err == 0 else np.inf))
            if not err <= tol:
                bad.append(f"row {i} (flags {fl}, step {step!r}): {k} = {got!r}, replay {exp!r}, off by {err:.3e} > {tol:.3e}")
        used = i + 1
        if advances == window and fl & DV_ADVANCE:
            break
    return bad, worst, advances, used


@pytest.mark.parametrize("form,spec", FORMS, ids=[f"{f}-{s[0][1]}pieces_first" for f, s in FORMS])
def test_traced_scalars_against_an_open_loop_replay(frx, sc, ob, monkeypatch, form, spec):
    cands = [sc.make_candidate(sid, N, gates, obstacles=obst) for sid, N, gates, obst in spec]
    prob = frx.Problem(cands, sc.ZHANGJIAJIE, qd_intervals=KAPPA)
    prob.set_resident(False)
    if form == "banded_lu":
        prob.set_solver("banded_lu")
    if form == "skip_inactive":
        monkeypatch.setenv("FRX_SKIP_INACTIVE", "1")
    prob.set_eval_solo(2 if form == "solo" else 0)
    if form == "solo":
        assert prob.eval_solo() >= 1
    x0 = prob.initial_guess()
    monkeypatch.setenv("FRX_TRACE", "1")
    r = prob.optimize(1e-6, x0=x0, max_iterations=30)
    monkeypatch.delenv("FRX_TRACE")
    assert r["resident"] == 0
    rows = prob.trace()
    prob.close()

    o = ob.Oracle(cands[0], sc.ZHANGJIAJIE, qd_intervals=KAPPA)
    o.set_abscissa_mode(False)
    assert o.n == int(prob.x_off[1] - prob.x_off[0])
    bad, worst, advances, used = replay(frx, o, x0[prob.x_off[0]:prob.x_off[1]], rows)
    print(f"{form} {[c[1] for c in spec]} pieces: {used} rows, {advances} advances; worst error / tolerance " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert not bad, "\n".join(bad[:8])
    assert advances == 10 and used >= 12, (advances, used, len(rows))
