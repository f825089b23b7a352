"""The 100 MHz stamps of cluster 0 during one evaluation in the one-launch form (frx_debug_profile_eval_cluster), in us after the leader's entry, median of 9:
40..43 leader entry / forward map done / adjoint done / end, 44..48 member 1 wave 0, the early-duration form's (forward_knot_body<.., ET>) 50..63, and the front of
the leader's wave 0: 32 tau load issued, 33 tau in its register.  The front's three intervals (entry -> tau issued -> landed -> durations formed) are medians of the
per-run differences.  Run it once per form (FRX_EVAL_EARLY_T=0 / 1).   python scripts/eval_early_timeline.py [config]"""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from frx_import import frx
from fast_racing_amd import scenario as sc
name = sys.argv[1] if len(sys.argv) > 1 else "headline"
B, N, gates, kappa = sc.CONFIGS[name]
prob = frx.Problem([sc.make_candidate(0, N, gates, perturb_id=b) for b in range(B)], sc.ZHANGJIAJIE, qd_intervals=kappa)
xs = prob.optimize(sc.ZHANGJIAJIE["opt_rel_tol"], x0=prob.initial_guess(), max_iterations=60)["x"]
names = {32: "leader wave 0 tau load issued", 33: "leader wave 0 tau in its register",
         40: "leader entry", 41: "leader forward map done", 42: "leader adjoint done", 43: "leader end", 44: "member 1 entry", 46: "member 1 samples start",
         47: "member 1 samples done", 48: "member 1 partials out", 50: "leader wave 0 durations formed", 51: "leader axis waves staged", 52: "leader waypoint map done",
         59: "leader matrix wave done", 60: "last member wave 0 durations formed", 61: "last member axis waves staged", 62: "last member waypoint map done", 63: "last member matrix wave done"}
names.update({53 + s: "leader matrix step %d done" % s for s in range(6)})
front = (("entry -> tau issued", 40, 32), ("tau issued -> landed", 32, 33), ("landed -> durations formed", 33, 50))
runs = []
for rep in range(9):
    st = prob.profile_eval_cluster(xs).astype(np.float64)
    runs.append({i: (st[i] - st[40]) / 100.0 for i in names if st[i] != 0})
keys = sorted(set.intersection(*[set(r) for r in runs]))
med = {k: float(np.median([r[k] for r in runs])) for k in keys}
out = {"config": name, "early_t": os.environ.get("FRX_EVAL_EARLY_T", "1"), "us_since_leader_entry": {f"{k}:{names[k]}": round(med[k], 2) for k in sorted(med, key=lambda q: med[q])}}
if all(a in med and b in med for _, a, b in front):
    out["front_us"] = {label: round(float(np.median([r[b] - r[a] for r in runs])), 2) for label, a, b in front}
    out["front_us_runs"] = {label: [round(r[b] - r[a], 2) for r in runs] for label, a, b in front}
print(json.dumps(out, indent=1))
