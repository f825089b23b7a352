"""The resident round kernel (csrc/frx_round_kernel.hpp: one launch per plan, compact-form L-BFGS direction from a register-resident
history, per-candidate mailboxes) against the one-launch-per-stage rounds (whose direction kernel is pinned to the host two-loop
recursion by frx_dv_selftest and whose evaluation kernels are pinned to the oracle).  Both run the SAME host state machines, so
command by command the scalars that cross the mailbox must agree to rounding until the path sensitivity of the optimisation
 takes over; complete plans must end with the same status and inside the CPU-vs-CPU' envelope."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _plan(prob, tol, resident, trace=False, **kw):
    prob.set_resident(resident)
    if trace:
        os.environ["FRX_TRACE"] = "1"
    try:
        r = prob.optimize(tol, **kw)
    finally:
        os.environ.pop("FRX_TRACE", None)
    r["trace"] = prob.trace() if trace else None
    return r


# (the last geometry: 17 candidates = eight workgroups per cluster, one piece per wave-task at kappa = 32 - 64 tasks in three passes over the cluster's 28
# waves, the LEADER's included: its waves write their partials' granules and then poll them like everybody else's)
@pytest.mark.parametrize("B,N,gates,kappa", [(3, 32, 8, 8), (1, 64, 16, 16), (2, 40, 10, 12), (17, 64, 16, 32)])
def test_resident_rounds_equal_per_stage_rounds(frx, sc, B, N, gates, kappa):
    cands = sc.make_batch(11, B, N, gates)
    prob = frx.Problem(cands, sc.ZHANGJIAJIE, qd_intervals=kappa)
    x0 = prob.initial_guess()
    a = _plan(prob, 1e-6, True, trace=True, x0=x0, max_iterations=40)
    b = _plan(prob, 1e-6, False, trace=True, x0=x0, max_iterations=40)
    assert a["resident"] >= 2 and a["device_status"] == 0, (a["resident"], a["device_status"])
    assert b["resident"] == 0
    ta, tb = a["trace"], b["trace"]
    rows = min(len(ta), len(tb), 30)
    assert rows >= 10, (len(ta), len(tb))
    worst = 0.0
    for i in range(rows):
        fa, fb = ta[i], tb[i]
        assert int(fa[0]) == int(fb[0]), f"command {i}: flags {fa[0]} vs {fb[0]}"
        scale_g = np.sqrt(max(fb[6], 1e-300))
        errs = [abs(fa[1] - fb[1]) / max(abs(fb[1]), 1e-300), abs(fa[2] - fb[2]) / abs(fb[2]), abs(fa[5] - fb[5]) / max(fb[5], 1e-300), abs(fa[6] - fb[6]) / max(fb[6], 1e-300)]
        if int(fb[0]) & 4:      # ADVANCE: the new direction's slope
            errs.append(abs(fa[4] - fb[4]) / max(abs(fb[4]), 1e-300))
        worst = max(worst, max(errs))
        assert max(errs) < 1e-8, f"command {i} (flags {int(fb[0])}): step/f/xx/gg[/dginit] rel err {errs}\nresident {fa}\nper-stage {fb}"
    print(f"B={B} N={N}: {rows} commands compared, worst relative difference {worst:.2e}; resident {a['ms_total']:.2f} ms vs per-stage {b['ms_total']:.2f} ms for {a['rounds']} rounds")
    assert np.abs(a["x"] - b["x"]).max() <= 1e-5 * np.abs(b["x"]).max()
    prob.close()


def _two_loop(S, Y, ys, g, newest, bound, m):
    """d = -H g by the reference's two-loop recursion (lbfgs.hpp:1381-1411): history slots S[j], Y[j] with ys[j] = y_j.s_j, `newest` the slot
    of the pair stored last, `bound` pairs in use; H0 = (y.s / y.y) I of the newest pair (lbfgs.hpp:1403)."""
    d = -g.copy()
    alpha = np.zeros(m)
    j = (newest + 1) % m
    for _ in range(bound):
        j = (j + m - 1) % m
        alpha[j] = (S[j] @ d) / ys[j]
        d -= alpha[j] * Y[j]
    d *= ys[newest] / (Y[newest] @ Y[newest])
    for _ in range(bound):
        beta = (Y[j] @ d) / ys[j]
        d += (alpha[j] - beta) * S[j]
        j = (j + 1) % m
    return d


@pytest.mark.parametrize("sid,N,gates,kappa,steps,chunk", [(0, 64, 16, 16, 420, 28), (4, 64, 16, 16, 330, 56), (4, 64, 16, 16, 330, 28)])
def test_resident_direction_equals_the_two_loop_recursion(frx, sc, monkeypatch, sid, N, gates, kappa, steps, chunk):
    """The resident kernel evaluates d = -H g in the compact (Byrd-Nocedal-Schnabel) form with an incrementally maintained R^-1
    (append a column per accepted step, drop a row and a column once the 128-pair history is full).  Contract: the reference's two-loop
    recursion (lbfgs.hpp:1381-1411).  Every accepted step of a headline-size candidate (n ~ 640 variables, m = 128) is logged on the
    device - the pair (s, y) handed to the cluster, the gradient and the direction that came back - and every direction is compared with
    a host recursion over the SAME pairs; the run is long enough for the history to wrap around at least twice."""
    m = 128
    # both size classes of the kernel: 28 history elements per thread (twelve history workgroups: what a batch of up to 16 headline candidates gets,
    # round 4) and 56 (six: the 32-candidate batch)
    monkeypatch.setenv("FRX_RESIDENT_E", str(chunk))
    cand = sc.make_candidate(sid, N, gates)
    prob = frx.Problem([cand], sc.ZHANGJIAJIE, qd_intervals=kappa)
    n = int(prob.x_off[1])
    assert n >= 2 * m
    prob.direction_log(steps + 8, 1)
    r = _plan(prob, 1e-12, True, max_iterations=steps)          # tolerance far below the stock one: the run ends at the iteration limit
    assert r["resident"] == (14 if chunk == 28 else 8) and r["device_status"] == 0
    log = prob.read_direction_log(0)
    rows = len(log["slot"])
    assert rows >= 300 and rows >= 2 * m + 40, rows
    S = np.zeros((m, n)); Y = np.zeros((m, n)); ys = np.zeros(m)
    worst, worst_at, cond_max = 0.0, -1, 0.0
    errs = []
    for k in range(rows):
        j, bound = int(log["slot"][k]), int(log["bound"][k])
        assert j == k % m and bound == min(k + 1, m), (k, j, bound)   # the reference's `end` / `bound` bookkeeping (lbfgs.hpp:1362-1379)
        S[j] = log["s"][k, :n]; Y[j] = log["y"][k, :n]; ys[j] = Y[j] @ S[j]
        assert not np.any(log["s"][k, n:]) and not np.any(log["d"][k, n:])
        d_ref = _two_loop(S, Y, ys, log["g"][k, :n], j, bound, m)
        err = np.abs(log["d"][k, :n] - d_ref).max() / np.abs(d_ref).max()
        errs.append(err)
        if err > worst:
            worst, worst_at = err, k
        if k % 16 == 15 or k == rows - 1:                          # condition number of the triangular factor the kernel keeps inverted
            order = [(j - a) % m for a in range(bound - 1, -1, -1)]   # oldest ... newest
            R = np.triu(S[order] @ Y[order].T)
            cond_max = max(cond_max, float(np.linalg.cond(R)))
    errs = np.array(errs)
    summary = {"scenario": sid, "n": n, "m": m, "accepted_steps": rows, "worst_rel_err": float(worst), "worst_at_step": worst_at,
               "median_rel_err": float(np.median(errs)), "rel_err_after_first_wrap": float(errs[m:].max()), "cond_R_max": cond_max}
    print(json.dumps(summary))
    os.makedirs(os.path.join(ROOT, "gpurun_out"), exist_ok=True)
    json.dump(summary, open(os.path.join(ROOT, "gpurun_out", f"direction_pin_s{sid}_e{chunk}.json"), "w"), indent=1)
    assert worst <= 1e-9, summary
    prob.direction_log(0, 0)
    prob.close()


def test_resident_plans_end_like_per_stage_plans(frx, sc, ob):
    """Stock tolerance, headline geometry (8 candidates x 64 pieces x kappa 16): same L-BFGS verdicts, objectives within the path
    sensitivity of the reference's stop rule - MEASURED HERE on the same candidates (the fixed 5e-3 of rounds 2-4 is gone): four CPU
    plans per candidate (both abscissa forms, x0 moved by a few ulp), tolerance = 1.5 x the largest spread among them - and bit-reproducible from call to call."""
    B, N, gates, kappa = 8, 64, 16, 16
    cands = [sc.make_candidate(0, N, gates, perturb_id=b) for b in range(B)]
    prob = frx.Problem(cands, sc.ZHANGJIAJIE, qd_intervals=kappa)
    tol = sc.ZHANGJIAJIE["opt_rel_tol"]
    a = _plan(prob, tol, True)
    a2 = _plan(prob, tol, True)
    b = _plan(prob, tol, False)
    assert a["resident"] >= 2 and a["device_status"] == 0 and b["resident"] == 0
    print(json.dumps({"resident_ms": a["ms_total"], "resident_rounds": a["rounds"], "per_stage_ms": b["ms_total"], "per_stage_rounds": b["rounds"],
                      "us_per_round_resident": 1e3 * a["ms_total"] / a["rounds"], "us_per_round_per_stage": 1e3 * b["ms_total"] / b["rounds"]}))
    assert np.array_equal(a["x"], a2["x"]) and np.array_equal(a["evals"], a2["evals"])        # deterministic: fixed-order reductions everywhere
    assert a["resident_retried"] == 0 and a["resident_failed"] == 0            # the resident kernel's own verdicts: nothing is re-run
    # the leaders ran the host's line search in step with it: rounds started on a predicted ADVANCE and on a predicted trial step, and the
    # host's command confirmed every single prediction (same source, no floating-point contraction on either side)
    adv, trial, redone = a["predictions"]
    print(json.dumps({"rounds_on_predicted_advance": adv, "rounds_on_predicted_trial_step": trial, "predictions_redone": redone, "evaluations": int(a["evals"].sum())}))
    assert adv > 0.5 * a["iters"].sum() and trial > 0 and redone == 0, a["predictions"]       # (8 candidates: the leaders also start on expected trial steps)
    assert np.array_equal(a["status"], b["status"]) and np.all(a["status"] >= 0)
    rel = np.abs(a["objective"] - b["objective"]) / np.abs(b["objective"])
    from test_gpu_configs import _cpu_plans
    cpu = _cpu_plans(ob, sc, cands, kappa, tol, [(False, 0), (True, 0), (False, 11), (False, 12)])
    assert all(p["status"] >= 0 for plans in cpu for p in plans)
    spread = np.array([(max(p["objective"] for p in plans) - min(p["objective"] for p in plans)) / abs(plans[0]["objective"]) for plans in cpu])
    # both device paths inside the CPU plans' own envelope as well (distance to the nearest CPU plan)
    near = lambda r: np.array([min(abs(r["objective"][i] - p["objective"]) for p in plans) / abs(plans[0]["objective"]) for i, plans in enumerate(cpu)])
    print(json.dumps({"resident_vs_per_stage_objective": {"max": float(rel.max()), "median": float(np.median(rel))}, "cpu_vs_cpu_spread": {"max": float(spread.max()), "median": float(np.median(spread))},
                      "resident_to_nearest_cpu_plan_max": float(near(a).max()), "per_stage_to_nearest_cpu_plan_max": float(near(b).max()), "tolerance": float(1.5 * spread.max())}))
    assert rel.max() <= 1.5 * spread.max(), (rel, spread)
    assert near(a).max() <= 1.5 * spread.max() and near(b).max() <= 1.5 * spread.max()
    prob.close()


@pytest.mark.parametrize("B", [1, 17])
def test_stock_kappa_48_plans_resident_like_per_stage(frx, sc, B):
    """BASELINE configs[0] geometry - 64 pieces at the STOCK QdIntervals = 48 (zhangjiajie_params.yaml; 49 samples per piece: one piece per wave-task, 64
    tasks).  One candidate (the reference's real use: 18 workgroups - the 64 tasks fit the 64 waves of its 16 history workgroups in one pass and the leader keeps
    its hands free for the adjoint; until round 5: 16 workgroups, two passes) and seventeen (ten workgroups per cluster - what three groups of eight clusters leave
    of 256 CUs: 64 tasks on 36 waves = TWO penalty passes per evaluation, the leader's waves included): the first commands agree with the per-stage path to rounding,
    the complete plans end with the same verdicts."""
    cands = [sc.make_candidate(0, 64, 16, perturb_id=b) for b in range(B)]
    prob = frx.Problem(cands, sc.ZHANGJIAJIE, qd_intervals=48)
    x0 = prob.initial_guess()
    a = _plan(prob, 1e-6, True, trace=True, x0=x0, max_iterations=40)
    b = _plan(prob, 1e-6, False, trace=True, x0=x0, max_iterations=40)
    assert a["resident"] == (18 if B == 1 else 10) and a["device_status"] == 0 and b["resident"] == 0, (a["resident"], a["device_status"])
    ta, tb = a["trace"], b["trace"]
    rows = min(len(ta), len(tb), 30)
    assert rows >= 10
    for i in range(rows):
        fa, fb = ta[i], tb[i]
        assert int(fa[0]) == int(fb[0]), f"command {i}: flags {fa[0]} vs {fb[0]}"
        errs = [abs(fa[1] - fb[1]) / max(abs(fb[1]), 1e-300), abs(fa[2] - fb[2]) / abs(fb[2]), abs(fa[5] - fb[5]) / max(fb[5], 1e-300), abs(fa[6] - fb[6]) / max(fb[6], 1e-300)]
        assert max(errs) < 1e-8, f"command {i}: {errs}"
    tol = sc.ZHANGJIAJIE["opt_rel_tol"]
    ra = _plan(prob, tol, True, x0=x0)
    rb = _plan(prob, tol, False, x0=x0)
    assert ra["resident"] > 0 and ra["device_status"] == 0 and rb["resident"] == 0
    assert np.array_equal(ra["status"] >= 0, rb["status"] >= 0) and np.all(ra["status"] >= 0)
    rel = np.abs(ra["objective"] - rb["objective"]) / np.abs(rb["objective"])
    print(json.dumps({"kappa": 48, "B": B, "resident_ms": ra["ms_total"], "resident_rounds": ra["rounds"], "us_per_round_resident": 1e3 * ra["ms_total"] / ra["rounds"],
                      "per_stage_ms": rb["ms_total"], "us_per_round_per_stage": 1e3 * rb["ms_total"] / rb["rounds"], "objective_rel_diff_max": float(rel.max())}))
    assert rel.max() < 5e-3, rel                                            # (independent runs of the reference's stop rule: DESIGN.md 4)
    prob.close()


def test_a_plan_that_ended_on_nan_leaves_nothing_behind_for_the_next_candidate_of_its_cluster(frx, sc, monkeypatch):
    """Work queue, one cluster: the infeasible scenario 170 (the reference algorithm "accepts" NaN objectives in its backtracking search; the host
    gives up after 64 of them - its accepted steps leave NaN pairs in the history registers) runs FIRST, two healthy candidates follow on the same
    cluster.  Their plans must be bit for bit the plans they get on clusters of their own: the new plan's first step wipes the slots (ADVICE r4;
    passes A and B multiply slots without a pair by zero, and 0 * NaN is NaN)."""
    cands = [sc.make_candidate(170, 64, 16), sc.make_candidate(3, 64, 16), sc.make_candidate(5, 64, 16)]
    tol = sc.ZHANGJIAJIE["opt_rel_tol"]
    prob = frx.Problem(cands, sc.ZHANGJIAJIE, qd_intervals=16)
    own = prob.optimize(tol)                                                # three clusters (bounded by the suite's iteration cap, tests/conftest.py)
    monkeypatch.setenv("FRX_RESIDENT_CLUSTERS", "1")
    q = prob.optimize(tol)                                                  # one cluster takes 170, then 3, then 5
    monkeypatch.delenv("FRX_RESIDENT_CLUSTERS")
    assert own["resident"] > 0 and q["resident"] > 0 and own["clusters"] == 3 and q["clusters"] == 1 and q["device_status"] == 0
    assert np.all(np.isfinite(q["objective"][1:])) and np.all(np.isfinite(q["x"][prob.x_off[1]:]))
    for key in ("status", "iters", "evals", "objective"):
        assert np.array_equal(q[key], own[key]), key
    assert np.array_equal(q["x"], own["x"])
    prob.close()


def test_shortcuts_of_the_round_kernel_do_not_change_a_plan(frx, sc, monkeypatch):
    """The leader's barrier-free confirmation and first-trial shortcut (FRX_RESIDENT_FAST_CONTROL) and the prediction levels
    (FRX_RESIDENT_SPECULATE) are ways to the SAME commands and the same arithmetic: with any of them switched off the plan is bit for bit the
    default one."""
    cands = [sc.make_candidate(0, 64, 16, perturb_id=b) for b in range(4)]
    prob = frx.Problem(cands, sc.ZHANGJIAJIE, qd_intervals=16)
    tol = sc.ZHANGJIAJIE["opt_rel_tol"]
    ref = _plan(prob, tol, True, max_iterations=600)
    assert ref["resident"] >= 3 and ref["device_status"] == 0
    for var, val in (("FRX_RESIDENT_FAST_CONTROL", "0"), ("FRX_RESIDENT_SPECULATE", "0"), ("FRX_RESIDENT_SPECULATE", "1")):
        monkeypatch.setenv(var, val)
        r = _plan(prob, tol, True, max_iterations=600)
        monkeypatch.delenv(var)
        assert r["device_status"] == 0 and r["resident"] == ref["resident"], (var, val)
        for key in ("x", "status", "iters", "evals", "objective"):
            assert np.array_equal(r[key], ref[key]), (var, val, key)
    prob.close()


def test_batches_larger_than_the_chip_take_the_work_queue_and_small_problems_the_per_stage_path(frx, sc, monkeypatch):
    cands = [sc.make_candidate(7, 32, 8, perturb_id=i) for i in range(70)]        # 70 clusters x >= 5 workgroups > 256 CUs
    prob = frx.Problem(cands, sc.ZHANGJIAJIE, qd_intervals=8)
    r = prob.optimize(1e-5, max_iterations=30)
    assert r["resident"] >= 3 and 0 < r["clusters"] < 70 and r["device_status"] == 0 and np.all(np.isfinite(r["objective"]))
    monkeypatch.setenv("FRX_RESIDENT_QUEUE", "0")                                 # the same batch, one launch per stage and round
    s = prob.optimize(1e-5, max_iterations=30)
    monkeypatch.delenv("FRX_RESIDENT_QUEUE")
    assert s["resident"] == 0 and np.array_equal(s["status"], r["status"]) and np.array_equal(s["evals"], r["evals"])
    assert np.max(np.abs(s["objective"] - r["objective"]) / np.abs(s["objective"])) < 1e-6
    prob.close()
    # fewer variables than twice the history length: the compact representation would invert an ill-conditioned R (frx_resident_plan.hpp)
    small = frx.Problem(sc.make_batch(2, 2, 5, 1), sc.ZHANGJIAJIE, qd_intervals=8)
    r = small.optimize(1e-6)
    assert r["resident"] == 0 and np.all(r["status"] >= 0)
    small.close()


def test_work_queue_plans_do_not_depend_on_the_cluster_that_runs_them(frx, sc, monkeypatch):
    """Seven candidates of DIFFERENT length on two clusters (FRX_RESIDENT_CLUSTERS): every cluster takes several candidates one after the
    other - longer after shorter and shorter after longer (the zero padding of the cluster's exchange buffers), a history that starts
    empty again - and every plan is bit for bit the plan of the same candidate on a cluster of its own."""
    Ns = [64, 40, 56, 64, 48, 36, 64]
    cands = [sc.make_candidate(20 + b, Ns[b], 8) for b in range(len(Ns))]
    prob = frx.Problem(cands, sc.ZHANGJIAJIE, qd_intervals=8)
    tol = sc.ZHANGJIAJIE["opt_rel_tol"]
    a = _plan(prob, tol, True)
    assert a["resident"] >= 3 and a["clusters"] == len(Ns) and a["device_status"] == 0
    for clusters in (2, 3):
        monkeypatch.setenv("FRX_RESIDENT_CLUSTERS", str(clusters))
        q = _plan(prob, tol, True)
        monkeypatch.delenv("FRX_RESIDENT_CLUSTERS")
        assert q["resident"] == a["resident"] and q["clusters"] == clusters and q["device_status"] == 0
        for key in ("x", "status", "iters", "evals", "objective"):
            assert np.array_equal(q[key], a[key]), key
        adv, trial, redone = q["predictions"]
        assert (adv, trial, redone) == tuple(a["predictions"]) and redone == 0
    prob.close()


def test_work_queue_at_the_headline_size(frx, sc, monkeypatch):
    """40 headline candidates = the chip's 32 clusters + 8 through the queue; the same plans as a batch of 32 and a batch of 8 (in the SAME size class
    of the kernel: a batch of 8 alone would get twelve history workgroups per candidate - another summation order)."""
    monkeypatch.setenv("FRX_RESIDENT_E", "56")
    B, N, gates, kappa = 40, 64, 16, 16
    cands = [sc.make_candidate(0, N, gates, perturb_id=b) for b in range(B)]
    tol = sc.ZHANGJIAJIE["opt_rel_tol"]
    prob = frx.Problem(cands, sc.ZHANGJIAJIE, qd_intervals=kappa)
    q = prob.optimize(tol)
    prob.close()
    assert q["resident"] >= 3 and q["clusters"] == 32 and q["device_status"] == 0
    parts = []
    for lo, hi in ((0, 32), (32, 40)):
        pb = frx.Problem(cands[lo:hi], sc.ZHANGJIAJIE, qd_intervals=kappa)
        parts.append(pb.optimize(tol))
        pb.close()
        assert parts[-1]["resident"] == q["resident"]
    for key in ("x", "status", "evals", "objective"):
        assert np.array_equal(q[key], np.concatenate([r[key] for r in parts])), key
    print(json.dumps({"queue_ms": q["ms_total"], "batches_ms": [r["ms_total"] for r in parts], "evals_max": int(q["evals"].max()), "evals_mean": float(q["evals"].mean())}))


def test_resident_kernel_handles_failing_and_finishing_candidates(frx, sc, ob):
    """An infeasible scenario (reference verdict LBFGSERR_MINIMUMSTEP: restore + stop) next to healthy ones of different length:
    clusters leave the chip one by one."""
    cands = [sc.make_candidate(170, 64, 16), sc.make_candidate(3, 64, 16), sc.make_candidate(5, 64, 16)]
    prob = frx.Problem(cands, sc.ZHANGJIAJIE, qd_intervals=16)
    r = _plan(prob, sc.ZHANGJIAJIE["opt_rel_tol"], True)
    assert r["resident"] >= 2 and r["device_status"] == 0
    assert r["status"][0] in (-1005, -1004, -1008) and r["objective"][0] > 1e8 and np.all(r["status"][1:] >= 0)     # failed line search; or the suite's iteration cap / the NaN guard
    assert r["resident_failed"] == int(r["status"][0] != -1004) and r["resident_retried"] == 0               # the verdict stands, like lbfgs_optimize's return code in the reference
    # the reported objective belongs to the returned point
    f, _ = prob.objective(r["x"])
    assert abs(f[0] - r["objective"][0]) <= 1e-9 * abs(f[0])
    prob.close()


def test_failed_candidates_get_a_second_chance_on_the_per_stage_rounds(frx, sc, monkeypatch):
    """frx_debug_set_resident_retry: every candidate the resident kernel failed on is planned again on the per-stage rounds, from its start point, and the others keep
    their resident result bit for bit.  The same three candidates as above; 1500 iterations let the infeasible one reach its own verdict on the resident kernel
    (a failed line search after 703 iterations; the iteration limit is never retried) and keep the three plans at half a second.  The per-stage rounds treat
    candidates independently, so the one planned again ends exactly as it does in a per-stage plan of the whole batch."""
    cands = [sc.make_candidate(170, 64, 16), sc.make_candidate(3, 64, 16), sc.make_candidate(5, 64, 16)]
    prob = frx.Problem(cands, sc.ZHANGJIAJIE, qd_intervals=16)
    x0, tol, cap = prob.initial_guess(), sc.ZHANGJIAJIE["opt_rel_tol"], 1500
    monkeypatch.setenv("FRX_RESIDENT_RETRY", "0")                         # no second chance, not even the targeted one: the resident kernel's own verdicts
    first = _plan(prob, tol, True, x0=x0, max_iterations=cap)
    monkeypatch.delenv("FRX_RESIDENT_RETRY")
    prob.set_resident_retry(True)
    second = _plan(prob, tol, True, x0=x0, max_iterations=cap)
    prob.set_resident_retry(False)
    per_stage = _plan(prob, tol, False, x0=x0, max_iterations=cap)
    again = [b for b in range(3) if first["status"][b] < 0 and first["status"][b] != -1004]
    print(json.dumps({"first": first["status"].tolist(), "second": second["status"].tolist(), "per_stage": per_stage["status"].tolist(), "planned_again": again,
                      "evals": [first["evals"].tolist(), second["evals"].tolist(), per_stage["evals"].tolist()], "ms": [first["ms_total"], second["ms_total"], per_stage["ms_total"]]}))
    assert first["resident"] >= 2 and first["device_status"] == 0 and first["resident_retried"] == 0 and per_stage["resident"] == 0
    assert first["status"][0] not in (0, -1004) and 0 in again                                                 # the test is about a candidate that IS planned again
    assert second["resident_retried"] == len(again) >= 1
    assert second["resident"] == first["resident"] and second["taken_over"] == first["taken_over"] == 0 and second["device_status"] == 0
    seg = lambda r, b: r["x"][prob.x_off[b]:prob.x_off[b + 1]]
    for b in range(3):
        ref = per_stage if b in again else first
        assert np.array_equal(seg(second, b), seg(ref, b)) and second["status"][b] == ref["status"][b] and second["evals"][b] == ref["evals"][b], b
        if b not in again:
            assert second["iters"][b] == first["iters"][b] and second["objective"][b] == first["objective"][b], b
    prob.close()


def test_size_classes_of_the_kernel_agree(frx, sc, monkeypatch):
    """A batch that leaves the chip room (<= 16 headline candidates) runs with 28 history elements per thread on twelve history workgroups, a full
    batch with 56 on six: two summation orders of the same direction - same verdicts, objectives as close as two independent runs are."""
    cands = [sc.make_candidate(0, 64, 16, perturb_id=b) for b in range(4)]
    tol = sc.ZHANGJIAJIE["opt_rel_tol"]
    res = {}
    for chunk in (28, 56):
        monkeypatch.setenv("FRX_RESIDENT_E", str(chunk))
        prob = frx.Problem(cands, sc.ZHANGJIAJIE, qd_intervals=16)
        res[chunk] = prob.optimize(tol)
        prob.close()
    a, b = res[28], res[56]
    assert a["resident"] == 14 and b["resident"] == 8 and a["device_status"] == 0 and b["device_status"] == 0
    assert np.array_equal(a["status"] >= 0, b["status"] >= 0)
    assert np.abs(a["objective"] / b["objective"] - 1).max() < 5e-3


@pytest.mark.parametrize("chunk", [28, 56])
def test_cross_xcd_form_of_the_hand_offs_gives_the_same_plan(frx, sc, monkeypatch, chunk):
    """A cluster that finds its workgroups on ONE XCD uses plain stores for what it hands to its neighbours, any other cluster write-through (atomic)
    stores - including the two words of every granule (rk_ll_put).  On the test box every cluster sits on one XCD, so the other form would never
    run: FRX_RESIDENT_WRITE_THROUGH=1 makes every cluster take it.  Same arithmetic, other transport: the plans are bit-identical."""
    cands = [sc.make_candidate(0, 64, 16, perturb_id=b) for b in range(3)]
    tol = sc.ZHANGJIAJIE["opt_rel_tol"]
    monkeypatch.setenv("FRX_RESIDENT_E", str(chunk))
    out = []
    for wt in ("0", "1"):
        monkeypatch.setenv("FRX_RESIDENT_WRITE_THROUGH", wt)
        prob = frx.Problem(cands, sc.ZHANGJIAJIE, qd_intervals=16)
        out.append(prob.optimize(tol, max_iterations=1500))
        prob.close()
    a, b = out
    assert a["resident"] > 0 and b["resident"] > 0 and a["device_status"] == 0 and b["device_status"] == 0
    assert np.array_equal(a["x"], b["x"]) and np.array_equal(a["status"], b["status"]) and np.array_equal(a["evals"], b["evals"])


def test_more_than_64_pieces_take_the_per_stage_rounds(frx, sc):
    """The leader keeps the candidate's (C, T), x, polytopes, direction and reduction multipliers in LDS; with the 128-row knot arrays of 65 ... 128
    pieces that does not fit the CU's 160 KB, so such plans run as per-stage rounds (resident == 0) - silently, with the same result as with the
    resident kernel switched off.  (Should a geometry of that class ever fit, the generic instantiation of the round kernel takes it and the
    scalars crossing the mailbox must equal the per-stage path's, as for the small geometries.)"""
    cands = sc.make_batch(13, 1, 100, 20)
    prob = frx.Problem(cands, sc.ZHANGJIAJIE, qd_intervals=8)
    x0 = prob.initial_guess()
    a = _plan(prob, 1e-6, True, trace=True, x0=x0, max_iterations=30)
    b = _plan(prob, 1e-6, False, trace=True, x0=x0, max_iterations=30)
    assert b["resident"] == 0 and a["device_status"] == 0
    if a["resident"] == 0:
        assert np.array_equal(a["x"], b["x"]) and np.array_equal(a["status"], b["status"]) and np.array_equal(a["evals"], b["evals"])
    else:
        ta, tb = a["trace"], b["trace"]
        rows = min(len(ta), len(tb), 30)
        assert rows >= 10
        for i in range(rows):
            fa, fb = ta[i], tb[i]
            assert int(fa[0]) == int(fb[0]), f"command {i}: flags {fa[0]} vs {fb[0]}"
            errs = [abs(fa[1] - fb[1]) / max(abs(fb[1]), 1e-300), abs(fa[2] - fb[2]) / abs(fb[2]), abs(fa[5] - fb[5]) / max(fb[5], 1e-300), abs(fa[6] - fb[6]) / max(fb[6], 1e-300)]
            assert max(errs) < 1e-8, f"command {i}: {errs}"
        assert np.abs(a["x"] - b["x"]).max() <= 1e-5 * np.abs(b["x"]).max()
    prob.close()


def test_penalty_partials_as_granules_or_through_the_plain_array(frx, sc, monkeypatch):
    """The penalty partials reach the adjoint as granules that its lanes poll (<= 64 pieces) or - FRX_RESIDENT_NO_LL20=1, and the form every larger
    geometry would take - through the plain array behind the arrival count.  Other transport, same values: bit-identical plans."""
    cands = [sc.make_candidate(0, 64, 16, perturb_id=b) for b in range(3)]
    tol = sc.ZHANGJIAJIE["opt_rel_tol"]
    out = []
    for plain in (None, "1"):
        if plain: monkeypatch.setenv("FRX_RESIDENT_NO_LL20", plain)
        prob = frx.Problem(cands, sc.ZHANGJIAJIE, qd_intervals=16)
        out.append(prob.optimize(tol, max_iterations=1500))
        prob.close()
    a, b = out
    assert a["resident"] > 0 and b["resident"] > 0 and a["device_status"] == 0 and b["device_status"] == 0
    assert np.array_equal(a["x"], b["x"]) and np.array_equal(a["status"], b["status"]) and np.array_equal(a["evals"], b["evals"])
