"""The hand-off of the penalty partials in the one-launch evaluation: 100 MHz stamps of cluster 0 (frx_debug_profile_eval_tail), in us after the leader's entry, median of 9.
Member 1, wave 0: 46 samples start, 47 samples done, 69 the gate word's value has arrived, 48 partials out.  Leader: 70 / 71 wave 0 enters / has left its poll for the
partials, 72 / 73 axis wave 1 the same, 74 axis wave 1's Hermite adjoint done, 64 wave 0 behind the barrier that follows the knot adjoint, 43 end; 75 / 76 are the
spins of lane 0 of wave 0 / of axis wave 1.  The stretches the hand-off is judged by follow the stamps.  One form per process (the switches are read once):
FRX_EVAL_HANDOFF=0 = piece-major granules, 8-byte polls, the adjoint's multipliers requested behind the poll; FRX_EVAL_EARLY_T=0 = the staged form of the forward map.
   python scripts/eval_handoff_timeline.py [config]"""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from frx_import import frx
from fast_racing_amd import scenario as sc
name = sys.argv[1] if len(sys.argv) > 1 else "headline"
B, N, gates, kappa = sc.CONFIGS[name]
prob = frx.Problem([sc.make_candidate(0, N, gates, perturb_id=b) for b in range(B)], sc.ZHANGJIAJIE, qd_intervals=kappa)
xs = prob.optimize(sc.ZHANGJIAJIE["opt_rel_tol"], x0=prob.initial_guess(), max_iterations=60)["x"]
names = {40: "leader entry", 41: "leader forward map done", 46: "member 1 samples start", 47: "member 1 samples done", 69: "member 1 gate word arrived", 48: "member 1 partials out",
         70: "wave 0 enters the poll", 71: "wave 0 poll left", 72: "axis wave 1 enters the poll", 73: "axis wave 1 poll left", 74: "axis wave 1 Hermite adjoint done",
         64: "wave 0 behind the knot adjoint's barrier", 43: "leader end"}
runs, spins = [], []
for rep in range(9):
    st = prob.profile_eval_tail(xs).astype(np.float64)
    runs.append({i: (st[i] - st[40]) / 100.0 for i in names if st[i] != 0})
    spins.append((st[75], st[76]))
keys = sorted(set.intersection(*[set(r) for r in runs]))
med = {k: float(np.median([r[k] for r in runs])) for k in keys}
d = lambda a, b: round(float(np.median([r[b] - r[a] for r in runs])), 2)
print(json.dumps({"config": name, "handoff": os.environ.get("FRX_EVAL_HANDOFF", "1"), "early_t": os.environ.get("FRX_EVAL_EARLY_T", "1"),
                  "us_since_leader_entry": {f"{k}:{names[k]}": round(med[k], 2) for k in sorted(med, key=lambda q: (med[q], q))},
                  "samples_done_to_gate_word_us": d(47, 69), "gate_word_to_partials_out_us": d(69, 48), "samples_done_to_partials_out_us": d(47, 48),
                  "partials_out_to_wave0_poll_left_us": d(48, 71), "partials_out_to_axis_poll_left_us": d(48, 73), "axis_poll_left_to_hermite_done_us": d(73, 74),
                  "spins_wave0_lane0": float(np.median([s[0] for s in spins])), "spins_axis1_lane0": float(np.median([s[1] for s in spins]))}, indent=1))
