"""The adjoint solve mu = K^-1 wbar of the one-launch evaluation's leader, step by step: stamps of axis wave 1 of cluster 0 (frx_debug_profile_eval_tail), median and
mean over the repetitions.  100 MHz counter: 74 Hermite adjoint done, 34 + s step s of the solve done (s = 0..5, strides 1..32), 64 wave 0 behind the barrier that
follows the knot adjoint, 43 leader end - all in us after the leader's entry (40).  Shader clock: 26 -> 27 the solve, 27 -> 28 the knot adjoint behind it, in cycles.
The forward map: 50 + 9 matrix wave done (workgroup 0), 46 the first member's samples start.  One form per process (the switches are read once); AB_ROOT=<dir> loads
the package of another build.
   python scripts/eval_exchange_timeline.py [config] [reps]"""
import json, os, sys
sys.path.insert(0, os.path.abspath(os.environ.get("AB_ROOT", os.path.dirname(os.path.dirname(os.path.abspath(__file__))))))
import numpy as np
from frx_import import frx
from fast_racing_amd import scenario as sc
name = sys.argv[1] if len(sys.argv) > 1 else "headline"
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 9
B, N, gates, kappa = sc.CONFIGS[name]
prob = frx.Problem([sc.make_candidate(0, N, gates, perturb_id=b) for b in range(B)], sc.ZHANGJIAJIE, qd_intervals=kappa)
xs = prob.optimize(sc.ZHANGJIAJIE["opt_rel_tol"], x0=prob.initial_guess(), max_iterations=60)["x"]
runs = [prob.profile_eval_tail(xs).astype(np.float64) for _ in range(reps)]
wall = lambda a, b: [(st[b] - st[a]) / 100.0 for st in runs]
cyc = lambda a, b: [st[b] - st[a] for st in runs]
both = lambda v, nd: {"median": round(float(np.median(v)), nd), "mean": round(float(np.mean(v)), nd)}
have_steps = all(st[34 + s] != 0 for st in runs for s in range(6))
out = {"config": name, "reps": reps, "root": os.environ.get("AB_ROOT", "."), "handoff": os.environ.get("FRX_EVAL_HANDOFF", "1"), "early_t": os.environ.get("FRX_EVAL_EARLY_T", "1"),
       "us_since_leader_entry": {k: both(wall(40, s), 3) for k, s in (("matrix wave done", 59), ("member 1 samples start", 46), ("axis wave 1 poll left", 73), ("hermite adjoint done", 74),
                                                                      ("wave 0 behind the knot adjoint's barrier", 64), ("leader end", 43))},
       "hermite_done_to_barrier_us": both(wall(74, 64), 3), "matrix_done_to_samples_start_us": both(wall(59, 46), 3),
       "solve_cycles_26_27": both(cyc(26, 27), 0), "knot_adjoint_cycles_27_28": both(cyc(27, 28), 0)}
if have_steps:
    prev = 74
    out["solve_step_us"] = {}
    for s in range(6):
        out["solve_step_us"][f"stride {1 << s}"] = both(wall(prev, 34 + s), 3)
        prev = 34 + s
    out["hermite_done_to_solve_done_us"] = both(wall(74, 39), 3)
    out["solve_done_to_barrier_us"] = both(wall(39, 64), 3)
print(json.dumps(out, indent=1))
prob.close()
