"""The tail of one evaluation in the one-launch form: 100 MHz stamps of cluster 0's leader (frx_debug_profile_eval_tail), in us after the leader's entry, median of 9.
64 wave 0 behind the barrier that follows the knot adjoint, 65 wave 0's last gradient store issued, 66 axis wave 1's last store issued, 67 thread 0 has the verdict,
68 thread 0 has issued `done`; next to them 41..43 (forward map done, thread 0 out of the adjoint, end) and member 1's 48 (partials out).  The last line is what the
issue's gate asks for: from the barrier's exit to the workgroup's last stamped moment, less wave 0's own stretch from the barrier to its last store.
Run it once per form (FRX_EVAL_TAIL=0: f and `done` behind a workgroup barrier and a trip to the status word; default: from inside the adjoint).
   python scripts/eval_tail_timeline.py [config]"""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from frx_import import frx
from fast_racing_amd import scenario as sc
name = sys.argv[1] if len(sys.argv) > 1 else "headline"
B, N, gates, kappa = sc.CONFIGS[name]
prob = frx.Problem([sc.make_candidate(0, N, gates, perturb_id=b) for b in range(B)], sc.ZHANGJIAJIE, qd_intervals=kappa)
xs = prob.optimize(sc.ZHANGJIAJIE["opt_rel_tol"], x0=prob.initial_guess(), max_iterations=60)["x"]
names = {40: "leader entry", 41: "leader forward map done", 48: "member 1 partials out", 64: "wave 0 behind the knot adjoint's barrier", 65: "wave 0 last gradient store issued",
         66: "axis wave 1 last store issued", 67: "thread 0 verdict known", 68: "thread 0 done issued", 42: "thread 0 out of the adjoint", 43: "leader end"}
runs = []
for rep in range(9):
    st = prob.profile_eval_tail(xs).astype(np.float64)
    runs.append({i: (st[i] - st[40]) / 100.0 for i in names if st[i] != 0})
keys = sorted(set.intersection(*[set(r) for r in runs]))
med = {k: float(np.median([r[k] for r in runs])) for k in keys}
last = max(med[k] for k in (65, 66, 68))
print(json.dumps({"config": name, "tail": os.environ.get("FRX_EVAL_TAIL", "1"), "us_since_leader_entry": {f"{k}:{names[k]}": round(med[k], 2) for k in sorted(med, key=lambda q: (med[q], q))},
                  "barrier_exit_to_last_stamp_us": round(last - med[64], 2), "of_which_wave0_to_its_last_store_us": round(med[65] - med[64], 2)}, indent=1))
