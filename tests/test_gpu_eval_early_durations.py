"""The early-duration form of the one-launch evaluation (k_eval_cluster<.., ET = true>: wave 0 forms the durations from tau in registers, the axis waves stage and
meet at LDS counters, no workgroup barrier in front of the coefficient collection) against the staged form (FRX_EVAL_EARLY_T=0): only the order of loads and the
synchronisation differ, so f and grad f must be the same BITS.  The switch is read once per process: each form runs in a child process of its own."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r'''
import sys, json
sys.path.insert(0, sys.argv[1])
import numpy as np
from frx_import import frx
from fast_racing_amd import scenario as sc
out = {}
def run(name, prob, xs_list, stage_check=True):
    rows = [{"fused": prob.eval_fused()}]
    for x in xs_list:
        f, g = prob.objective(x)
        row = {"f": f.tobytes().hex(), "g": g.tobytes().hex()}
        if stage_check:
            prob.set_eval_fused(False)
            fs, _ = prob.objective(x)
            prob.set_eval_fused(True)
            row["f_equals_stage"] = bool(np.array_equal(f, fs))
        rows.append(row)
    out[name] = rows
    prob.close()
def points(prob, seed):
    x0 = prob.initial_guess()
    rng = np.random.default_rng(seed)
    return [x0, x0 + 0.05 * rng.standard_normal(x0.size)]
for name in ("headline", "plumbing", "synthetic8"):
    B, N, gates, kappa = sc.CONFIGS[name]
    cands = [sc.make_candidate(0, N, gates, perturb_id=b) for b in range(B)]
    prob = frx.Problem(cands, sc.ZHANGJIAJIE, qd_intervals=kappa)
    xs = points(prob, 1)
    xs.append(prob.optimize(sc.ZHANGJIAJIE["opt_rel_tol"], x0=xs[0], max_iterations=30)["x"])
    run(name, prob, xs)
for c2 in (1, 0):                                                   # fixed total time: the serial sums of forwardT inside wave 0
    prob = frx.Problem(sc.make_batch(0, 2, 16, 4), sc.ZHANGJIAJIE, qd_intervals=8, rho=0.0, total_t=9.0, c2_diffeo=c2)
    run("fixed_total_time_c2_%d" % c2, prob, points(prob, 5))
for N in (2, 3, 4, 5):                                              # zero, one, two and two reduction steps of the matrix wave
    prob = frx.Problem(sc.make_batch(0, 2, N, 0), sc.ZHANGJIAJIE, qd_intervals=8)
    run("pieces_%d" % N, prob, points(prob, 7))
specs = [(11, 8, 2, False), (12, 20, 5, True), (13, 1, 0, False), (14, 33, 8, True), (15, 2, 0, False)]
for over in ({}, dict(grid_res=1.7)):                              # ragged batches, split polytopes
    cands = [sc.make_candidate(sid, N, g, obstacles=o) for sid, N, g, o in specs]
    prob = frx.Problem(cands, sc.ZHANGJIAJIE, qd_intervals=8, **over)
    run("ragged" + ("_split" if over else ""), prob, points(prob, 9))
print(json.dumps(out))
'''


def _child(env_over):
    env = dict(os.environ)
    env.update(env_over)
    p = subprocess.run([sys.executable, "-c", CHILD, ROOT], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900, env=env)
    assert p.returncode == 0, p.stderr[-2000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("wt", ["0", "1"])
def test_early_durations_bit_identical_to_staged_form(wt):
    new = _child({"FRX_EVAL_EARLY_T": "1", "FRX_EVAL_FUSED_WT": wt})
    old = _child({"FRX_EVAL_EARLY_T": "0", "FRX_EVAL_FUSED_WT": wt})
    assert sorted(new) == sorted(old)
    for name in ("headline", "plumbing", "synthetic8", "fixed_total_time_c2_1", "pieces_3", "ragged"):
        assert new[name][0]["fused"] > 0, name                        # the one-launch evaluation is what these cases exercise
    for name in new:
        assert new[name][0] == old[name][0]
        assert len(new[name]) == len(old[name])
        for i, (a, b) in enumerate(zip(new[name][1:], old[name][1:])):
            assert a["f"] == b["f"], (name, i, "f")
            assert a["g"] == b["g"], (name, i, "grad f")
            assert a["f_equals_stage"] == b["f_equals_stage"], (name, i, "f against the stage kernels")
            if name in ("headline", "plumbing", "synthetic8"):
                assert a["f_equals_stage"], (name, i, "f against the stage kernels")
