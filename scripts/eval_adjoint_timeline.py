"""The leader's adjoint in the one-launch evaluation, from the end of its forward map to the end of the kernel: 100 MHz stamps of cluster 0 (frx_debug_profile_eval_tail),
in us after the leader's entry, median over the repetitions - the stamps of scripts/eval_handoff_timeline.py, eval_exchange_timeline.py and eval_tail_timeline.py in one
table.  41 forward map done; 77 axis wave 1 has requested its waypoint-layer operands (only where Problem.eval_adjoint() is 1); 70 / 71 wave 0 enters / has left its
poll for the partials, 72 / 73 axis wave 1 the same; 48 the first member's partials out; 74 axis wave 1's Hermite adjoint done, 34 + s step s of its solve, 64 wave 0
behind the barrier that follows the knot adjoint, 65 / 66 wave 0's / axis wave 1's last store issued, 68 `done` issued, 43 end.  The stretches the issue of this form
asks for follow the table.  One form per process (FRX_EVAL_ADJOINT is read once); AB_ROOT=<dir> loads the package of another build.
   python scripts/eval_adjoint_timeline.py [config] [reps]"""
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
names = {41: "leader forward map done", 77: "axis wave 1 waypoint operands requested", 70: "wave 0 enters the poll", 72: "axis wave 1 enters the poll",
         48: "member 1 partials out", 71: "wave 0 poll left", 73: "axis wave 1 poll left", 74: "axis wave 1 Hermite adjoint done", 39: "axis wave 1 solve done",
         64: "wave 0 behind the knot adjoint's barrier", 65: "wave 0 last gradient store issued", 66: "axis wave 1 last store issued", 68: "thread 0 done issued", 43: "leader end"}
runs = []
for rep in range(reps):
    st = prob.profile_eval_tail(xs).astype(np.float64)
    runs.append({i: (st[i] - st[40]) / 100.0 for i in names if st[i] != 0})
keys = sorted(set.intersection(*[set(r) for r in runs]))
med = {k: float(np.median([r[k] for r in runs])) for k in keys}
d = lambda a, b: round(float(np.median([r[b] - r[a] for r in runs])), 3) if a in keys and b in keys else None
print(json.dumps({"config": name, "reps": reps, "root": os.environ.get("AB_ROOT", "."), "adjoint": prob.eval_adjoint() if hasattr(prob, "eval_adjoint") else 0,
                  "us_since_leader_entry": {f"{k}:{names[k]}": round(med[k], 2) for k in sorted(med, key=lambda q: (med[q], q))},
                  "forward_done_to_wave0_poll_entered_us": d(41, 70), "forward_done_to_axis_poll_entered_us": d(41, 72),
                  "partials_out_to_wave0_poll_left_us": d(48, 71), "partials_out_to_axis_poll_left_us": d(48, 73),
                  "axis_poll_left_to_solve_done_us": d(73, 39), "solve_done_to_barrier_us": d(39, 64),
                  "barrier_to_wave0_last_store_us": d(64, 65), "barrier_to_axis_last_store_us": d(64, 66), "barrier_to_done_us": d(64, 68), "barrier_to_end_us": d(64, 43)}))
prob.close()
