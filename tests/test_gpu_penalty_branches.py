"""Every device path of the penalty integrand (frx_math.hpp: penalty_sample) against the oracle on branch-isolated states
(tests/penalty_states.py): each of the five penalty terms alone and all together, corridor faces, edges and corners, the pre-reject
guard, K = 1 .. 40 half-spaces per piece with different K in one wave, and a corridor large enough to step the large-batch launch down.

  integrator   prob.penalty(T, C): k_penalty_lat, k_penalty (FRX_PENALTY_FORM=thr, a child process), k_penalty_lat2 in its two-phase and
               one-phase forms, FRX_PENALTY_WAVES = 1 .. 4, a PenaltyProblem on the same polytopes - 1e-9 per piece, inactive pieces zero;
  objective    prob.objective(x): k_eval_cluster, three launches, k_eval_solo, banded LU - as in test_stagewise_parity;
  resident     k_round against the per-stage rounds under tight limits, command by command;
  differences  central differences of the device's own cost against its gradient."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import penalty_states as ps  # noqa: E402
from test_penalty_branches_cpu import _fd_check, compare, oracle_penalty  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PER_EVAL_TOL = 1e-9
LARGE_P = 3200                     # pieces past the large-batch threshold at kappa = 16 (three pieces per wave, 1024 SIMDs)


def integrator_states(sc, ob, kappa):
    out = ps.limit_states(sc, ob, kappa, iterate=0) + ps.limit_states(sc, ob, kappa, iterate=15) + ps.corridor_states(sc, ob, kappa)
    for s in out:
        ps.check(s, sc.ZHANGJIAJIE)
    return out


@pytest.fixture(scope="module")
def states8(sc, ob):
    return integrator_states(sc, ob, 8)


@pytest.fixture(scope="module")
def states16(sc, ob):
    return integrator_states(sc, ob, 16)


def _refs(sc, ob, s):
    return [oracle_penalty(ob, sc, s, b) for b in range(len(s.cands))]


def check_penalty(name, s, got, refs, rep=1):
    """got = (cost, gdT, gdC) of the state's candidates replicated `rep` times; the first, a middle and the last replica are compared."""
    cost, gdT, gdC = got
    off = s.piece_off
    B, P = len(s.cands), off[-1]
    for r in sorted({0, rep // 2, rep - 1}):
        for b in range(B):
            sl = slice(r * P + off[b], r * P + off[b + 1])
            compare(f"{name} {s.name} replica {r} cand {b}", (cost[r * B + b], gdT[sl], gdC[6 * sl.start:6 * sl.stop]), refs[b], PER_EVAL_TOL,
                    s.T[off[b]:off[b + 1]])


def run_penalty(frx, sc, s, rep=1):
    prob = frx.Problem(s.cands * rep, sc.ZHANGJIAJIE, qd_intervals=s.kappa, **s.override)
    got = prob.penalty(np.tile(s.T, rep), np.tile(s.C.reshape(-1), rep))
    kernel = prob.penalty_kernel()
    prob.close()
    return got, kernel


@pytest.mark.parametrize("kappa", [8, 16])
def test_latency_integrator_on_every_branch(frx, sc, ob, states8, states16, kappa):
    for s in (states8 if kappa == 8 else states16):
        got, kernel = run_penalty(frx, sc, s)
        assert kernel == "frx::k_penalty_lat"
        check_penalty("k_penalty_lat", s, got, _refs(sc, ob, s))


@pytest.mark.parametrize("waves", [1, 2, 3, 4])
def test_waves_per_workgroup_on_every_branch(frx, sc, ob, states16, monkeypatch, waves):
    monkeypatch.setenv("FRX_PENALTY_WAVES", str(waves))
    for s in states16:
        got, kernel = run_penalty(frx, sc, s)
        assert kernel == ("frx::k_penalty_lat2" if waves == 4 else "frx::k_penalty_lat"), kernel
        check_penalty(f"W={waves}", s, got, _refs(sc, ob, s))


def test_large_batch_integrator_on_every_branch_in_both_forms(frx, sc, ob, states16, monkeypatch):
    """The states replicated past the large-batch threshold: k_penalty_lat2 two-phase, then the one-phase launch on the same handle."""
    for s in states16:
        rep = -(-LARGE_P // s.piece_off[-1])
        prob = frx.Problem(s.cands * rep, sc.ZHANGJIAJIE, qd_intervals=s.kappa, **s.override)
        assert prob.penalty_kernel() == "frx::k_penalty_lat2"
        Tb, Cb = np.tile(s.T, rep), np.tile(s.C.reshape(-1), rep)
        two = prob.penalty(Tb, Cb)
        monkeypatch.setenv("FRX_PENALTY_TWOPHASE", "0")
        assert prob.penalty_kernel() == "frx::k_penalty_lat"
        one = prob.penalty(Tb, Cb)
        monkeypatch.delenv("FRX_PENALTY_TWOPHASE")
        prob.close()
        refs = _refs(sc, ob, s)
        check_penalty("k_penalty_lat2", s, two, refs, rep)
        check_penalty("k_penalty_lat2 one-phase", s, one, refs, rep)


def test_large_corridor_steps_the_large_batch_launch_down(frx, sc, ob):
    """One piece of 260 half-spaces: the four-wave workgroup's corridor blocks no longer fit a CU, the launch takes fewer waves (k_penalty_lat)."""
    s = ps.big_K_state(sc, ob, 16)
    ps.check(s, sc.ZHANGJIAJIE)
    rep = -(-LARGE_P // s.piece_off[-1])
    got, kernel = run_penalty(frx, sc, s, rep)
    assert kernel == "frx::k_penalty_lat", kernel
    check_penalty("stepped-down", s, got, _refs(sc, ob, s), rep)


def test_penalty_problem_on_every_branch(frx, sc, ob, states16):
    for s in states16:
        polys = [h for c in s.cands for h in c.h_polys]
        pp = frx.PenaltyProblem(sc.ZHANGJIAJIE, [c.coarse_n for c in s.cands], list(range(len(polys))), polys, qd_intervals=s.kappa, **s.override)
        got = pp.penalty(s.T, s.C)
        pp.close()
        check_penalty("PenaltyProblem", s, got, _refs(sc, ob, s))


def _child_throughput_form(out_path):
    """(child process, FRX_PENALTY_FORM=thr) the throughput form on every state; results to out_path."""
    from frx_import import frx
    from fast_racing_amd import scenario as sc
    from oracle import binding as ob
    res = {}
    for kappa in (8, 16):
        for i, s in enumerate(integrator_states(sc, ob, kappa)):
            (cost, gdT, gdC), kernel = run_penalty(frx, sc, s)
            assert kernel == "frx::k_penalty", kernel
            res[f"{kappa}_{i}_c"], res[f"{kappa}_{i}_t"], res[f"{kappa}_{i}_g"] = cost, gdT, gdC
    np.savez(out_path, **res)


def test_throughput_integrator_on_every_branch(frx, sc, ob, states8, states16):
    """The form is chosen once per process: it runs in a child."""
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "thr.npz")
        code = (f"import sys; sys.path.insert(0, {ROOT!r}); sys.path.insert(0, {os.path.join(ROOT, 'tests')!r}); "
                f"import test_gpu_penalty_branches as t; t._child_throughput_form({out!r})")
        subprocess.run([sys.executable, "-c", code], check=True, env=dict(os.environ, FRX_PENALTY_FORM="thr"), timeout=300)
        d = np.load(out)
        for kappa, sts in ((8, states8), (16, states16)):
            for i, s in enumerate(sts):
                check_penalty("k_penalty", s, (d[f"{kappa}_{i}_c"], d[f"{kappa}_{i}_t"], d[f"{kappa}_{i}_g"]), _refs(sc, ob, s))


# ---- objective level ----
def _objective_check(name, prob, oracles, s, x):
    f, g = prob.objective(x)
    for b, o in enumerate(oracles):
        xs = s.x[b]
        f_ref, g_ref = o.objective(xs)
        assert abs(f[b] - f_ref) <= PER_EVAL_TOL * abs(f_ref), f"{name} {s.name} cand {b}: f {f[b]!r} vs {f_ref!r}"
        gerr = np.abs(g[prob.x_off[b]:prob.x_off[b + 1]] - g_ref).max()
        assert gerr <= PER_EVAL_TOL * max(np.abs(g_ref).max(), abs(f_ref)), f"{name} {s.name} cand {b}: gradient error {gerr:.3e}"


@pytest.mark.parametrize("kappa", [8, 16, 48])
def test_objective_on_every_branch_in_every_form(frx, sc, ob, kappa):
    for it in (0, 15):
        for s in ps.limit_states(sc, ob, kappa, iterate=it):
            ps.check(s, sc.ZHANGJIAJIE)
            prob = frx.Problem(s.cands, sc.ZHANGJIAJIE, qd_intervals=kappa, **s.override)
            oracles = [ob.Oracle(c, sc.ZHANGJIAJIE, qd_intervals=kappa, **s.override) for c in s.cands]
            for o in oracles:
                o.set_abscissa_mode(False)
            x = np.concatenate(s.x)
            if kappa == 8:
                assert prob.eval_fused() > 0
                _objective_check("k_eval_cluster", prob, oracles, s, x)
            prob.set_eval_fused(False)
            prob.set_eval_solo(0)
            _objective_check("three launches", prob, oracles, s, x)
            if kappa != 8:
                prob.set_eval_solo(2)
                assert prob.eval_solo() >= 1
                _objective_check("k_eval_solo", prob, oracles, s, x)
                prob.set_eval_solo(0)
            prob.set_solver("banded_lu")
            _objective_check("banded_lu", prob, oracles, s, x)
            prob.close()


# ---- resident rounds under tight limits ----
@pytest.mark.parametrize("B,N,gates,kappa", [(3, 32, 8, 8), (17, 64, 16, 32)])
def test_resident_rounds_equal_per_stage_rounds_under_tight_limits(frx, sc, B, N, gates, kappa):
    from test_gpu_resident import _plan
    over = dict(ps.TIGHT, safe_margin=0.6)
    cands = sc.make_batch(11, B, N, gates)
    prob = frx.Problem(cands, sc.ZHANGJIAJIE, qd_intervals=kappa, **over)
    x0 = prob.initial_guess()
    T0, C0 = prob.forward(x0)
    ps.check(ps.State("resident start", cands, over, kappa, T0, C0.reshape(-1, 3), ps.TERMS), sc.ZHANGJIAJIE)    # all five terms live from the start
    a = _plan(prob, 1e-6, True, trace=True, x0=x0, max_iterations=40)
    b = _plan(prob, 1e-6, False, trace=True, x0=x0, max_iterations=40)
    assert a["resident"] >= 2 and a["device_status"] == 0, (a["resident"], a["device_status"])
    assert b["resident"] == 0
    ta, tb = a["trace"], b["trace"]
    # the two paths start equal to the last bits and part by rounding that the optimisation amplifies: under these limits (all five terms live)
    # the difference grows about tenfold every four commands, from 1e-15 at the first to ~1e-8 by the 27th on 17 x 64 pieces; 20 commands stay
    # well inside 1e-8, while a wrong branch in either path shows in the first evaluation
    rows = min(len(ta), len(tb), 20)
    assert rows >= 10, (len(ta), len(tb))
    for i in range(rows):
        fa, fb = ta[i], tb[i]
        assert int(fa[0]) == int(fb[0]), f"command {i}: flags {fa[0]} vs {fb[0]}"
        errs = [abs(fa[1] - fb[1]) / max(abs(fb[1]), 1e-300), abs(fa[2] - fb[2]) / abs(fb[2]), abs(fa[5] - fb[5]) / max(fb[5], 1e-300), abs(fa[6] - fb[6]) / max(fb[6], 1e-300)]
        if int(fb[0]) & 4:
            errs.append(abs(fa[4] - fb[4]) / max(abs(fb[4]), 1e-300))
        assert max(errs) < 1e-8, f"command {i} (flags {int(fb[0])}): step/f/xx/gg[/dginit] rel err {errs}"
    assert np.abs(a["x"] - b["x"]).max() <= 1e-5 * np.abs(b["x"]).max()
    prob.close()


# ---- finite differences of the device's own cost ----
def test_device_gradient_matches_finite_differences_on_every_branch(frx, sc, ob):
    for s in ps.small_states(sc, ob):
        ps.check(s, sc.ZHANGJIAJIE, min_samples=2)
        prob = frx.Problem(s.cands, sc.ZHANGJIAJIE, qd_intervals=s.kappa, **s.override)

        def dev(T, Cf):
            cost, gdT, gdC = prob.penalty(T, Cf)
            return cost[0], gdT, gdC
        _fd_check(s.name, dev, s.T, s.C)
        prob.close()
