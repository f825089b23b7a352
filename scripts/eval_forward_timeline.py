"""The prelude of the one-launch evaluation's forward map, stretch by stretch: the 100 MHz stamps of cluster 0 (frx_debug_profile_eval_forward) in us after the leader's
entry (40), median of the repetitions, and the stretches between consecutive stamps of each wave as medians of the per-run differences.
  wave 0 of the leader        80 at the early barrier, 81 out of it, 82 tau in its register, 83 Tc written, 50 durations formed, 84 rows built and first inverse done,
                              53..58 matrix steps 0..5 done, 59 matrix wave done
  wave 0 of the last member   88..92 the same five, 60 its durations formed, 63 its matrix wave done
  axis wave 1 of the leader   96 last staging load issued, 97 out of the early barrier, 98 loads landed, 99 staging stores done, 51 every axis wave staged, 100 vertex
                              trips done, 101 division done, 52 waypoint map done and durations seen, 102 right-hand side built, 103..108 steps 0..5 done, 109 final
                              multipliers seen, 110 coefficients written
  and 32 / 33 tau issued / landed, 41 forward map done, 46 member 1 samples start, 48 its partials out, 43 leader end.
One form per process (FRX_EVAL_PRELUDE is read once); AB_ROOT=<dir> loads the package of another build.
   python scripts/eval_forward_timeline.py [config] [reps]"""
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
chains = {
    "leader wave 0": [(40, "entry"), (32, "tau issued"), (33, "tau landed"), (80, "at the early barrier"), (81, "out of it"), (82, "tau in its register"), (83, "Tc written"),
                      (50, "durations formed"), (84, "rows built, first inverse")] + [(53 + s, "matrix step %d" % s) for s in range(6)] + [(59, "matrix wave done")],
    "last member wave 0": [(88, "at the early barrier"), (89, "out of it"), (90, "tau in its register"), (91, "Tc written"), (60, "durations formed"), (92, "rows built, first inverse"),
                           (63, "matrix wave done")],
    "leader axis wave 1": [(96, "last staging load issued"), (97, "out of the early barrier"), (98, "loads landed"), (99, "staging stores done"), (51, "axis waves staged"),
                           (100, "vertex trips done"), (101, "division done"), (52, "waypoint map done"), (102, "right-hand side built")]
                          + [(103 + s, "step %d" % s) for s in range(6)] + [(109, "final multipliers seen"), (110, "coefficients written")],
    "behind the forward map": [(41, "leader forward map done"), (46, "member 1 samples start"), (48, "member 1 partials out"), (43, "leader end")],
}
runs = [prob.profile_eval_forward(xs).astype(np.float64) for _ in range(reps)]
out = {"config": name, "reps": reps, "root": os.environ.get("AB_ROOT", "."), "prelude": prob.eval_prelude(), "us_since_leader_entry": {}, "stretch_us": {}}
for wave, slots in chains.items():
    have = [(i, label) for i, label in slots if all(st[i] != 0 for st in runs)]
    out["us_since_leader_entry"][wave] = {f"{i}:{label}": round(float(np.median([(st[i] - st[40]) / 100.0 for st in runs])), 2) for i, label in have}
    if wave != "behind the forward map":
        out["stretch_us"][wave] = {f"{la} -> {lb}": round(float(np.median([(st[b] - st[a]) / 100.0 for st in runs])), 2) for (a, la), (b, lb) in zip(have, have[1:])}
print(json.dumps(out, indent=1))
prob.close()
