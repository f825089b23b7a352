"""The compile-time geometry class of the one-launch evaluation (k_eval_cluster<.., EvalGeomK16>, frx_eval_kernel.hpp): 17 samples per piece, 3 pieces per wave-task,
corridor blocks of 8 half-spaces, six reduction steps as integer constants.  Only integers, strides and trip counts differ from the run-time instantiation
(FRX_EVAL_GEOM=0), so f and the gradient are the same BITS; the switch is read once per process, so the forms are compared between child processes started fresh, and
Problem.eval_geometry() says which instantiation a handle launches.

Which handles qualify: kappa = 16 (17 samples per piece, 3 pieces per wave-task), the synthetic corridor (boxes of 6 faces joined pairwise: Kmax = 8) and a longest candidate
of 34..64 pieces (six reduction steps).  So (64,), the ragged handle and the nine candidates qualify as they are; (3,) and (2,) alone have one reduction step or none and
take the run-time form - they are checked as such, and next to a 64-piece candidate, (64, 3) and (64, 2), where they run through the class: the first lane shift and the
single waypoint inside a wave-task of one piece, nst = 1 and 0 under the class's six steps.  N stays per candidate: the ragged candidates of 7, 9, 3 and 2 pieces have
partial wave-tasks and nst from 1 to 3.
Handles that must NOT take the class: kappa = 8, kappa = 48 with one candidate, a longest candidate of 32 pieces (five steps), a corridor with obstacle planes (Kmax != 8)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRAD_TOL = 1e-10           # one launch against three stage launches, per candidate: |g1 - g3|max <= 1e-10 max(|g3|max, |f3|) - the bound of tests/test_gpu_parity.py for these two forms

# name: (pieces per candidate, samples per piece - 1, corridor with obstacle planes, takes the class)
SHAPES = {
    "full": ((64,), 16, False, 1),
    "ragged": ((64, 7, 9, 3, 2), 16, False, 1),
    "first_lane_shift": ((3,), 16, False, 0),
    "one_waypoint": ((2,), 16, False, 0),
    "first_lane_shift_beside_64": ((64, 3), 16, False, 1),
    "one_waypoint_beside_64": ((64, 2), 16, False, 1),
    "nine_clusters": ((64, 5, 12, 3, 33, 64, 8, 2, 17), 16, False, 1),
    "kappa8": ((64, 14, 10, 7, 2), 8, False, 0),
    "kappa48_one_candidate": ((64,), 48, False, 0),
    "five_steps": ((32, 7, 3), 16, False, 0),
    "obstacle_planes": ((64, 7), 16, True, 0),
}
# the duration layers as tests/test_gpu_parity.py builds them: soft total time (the default), fixed total time
LAYERS = {
    "soft": {},
    "fixed": {"rho": 0.0, "total_t": 9.0, "c2_diffeo": 1},
}
CASES = [f"{s}-{l}" for s in SHAPES for l in LAYERS]
CLASS_CASES = [c for c in CASES if SHAPES[c.split("-")[0]][3]]

CHILD = r'''
import json, sys
sys.path.insert(0, sys.argv[1])
import numpy as np
from frx_import import frx
from fast_racing_amd import scenario as sc
shapes, layers = json.loads(sys.argv[2]), json.loads(sys.argv[3])
out = {}
for sname, (pieces, kappa, obstacles, _) in shapes.items():
    for lname, over in layers.items():
        cands = [sc.make_candidate(0, n, n // 4 if n >= 8 else 0, perturb_id=b, obstacles=bool(obstacles)) for b, n in enumerate(pieces)]
        prob = frx.Problem(cands, sc.ZHANGJIAJIE, qd_intervals=kappa, **over)
        x = prob.initial_guess() + 1e-3 * np.sin(np.arange(prob.NX))
        f, g = prob.objective(x)
        f2, g2 = prob.objective(x)                                   # the second evaluation on the handle
        out[sname + "-" + lname] = {"G": prob.eval_fused(), "geom": prob.eval_geometry(), "Kmax": prob.Kmax, "f": f.tobytes().hex(), "g": g.tobytes().hex(),
                                    "f2": f2.tobytes().hex(), "g2": g2.tobytes().hex()}
        prob.close()
print(json.dumps(out))
'''


def _child(extra_env):
    env = dict(os.environ)
    for k in ("FRX_EVAL_GEOM", "FRX_EVAL_CHAIN", "FRX_EVAL_HANDOFF", "FRX_EVAL_TAIL", "FRX_EVAL_EARLY_T", "FRX_EVAL_ARGPTR", "FRX_EVAL_FUSED", "FRX_EVAL_FUSED_WT"):
        env.pop(k, None)
    env.update(extra_env)
    p = subprocess.run([sys.executable, "-c", CHILD, ROOT, json.dumps(SHAPES), json.dumps(LAYERS)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=240, env=env)
    assert p.returncode == 0, p.stderr[-2000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


_forms = {}


def form(key):
    """(f, grad f) bits of every case from one fresh process per value of the switch; computed once, never changed."""
    if key not in _forms:
        _forms[key] = _child({"default": {}, "geom0": {"FRX_EVAL_GEOM": "0"}}[key])
    return _forms[key]


@pytest.mark.parametrize("case", CASES)
def test_bits_of_the_class_and_the_run_time_form(case):
    """Default against FRX_EVAL_GEOM=0: the same bits in f and in the gradient on the first and on the second evaluation of a handle; the query reports the class in the
    default process exactly for the handles that qualify, and the run-time form for every handle under the switch."""
    a, b = form("default")[case], form("geom0")[case]
    takes = SHAPES[case.split("-")[0]][3]
    assert a["G"] == b["G"] > 0, "the one-launch form is not in use"
    assert a["geom"] == takes and b["geom"] == 0, (case, a["geom"], b["geom"])
    if case.startswith("obstacle_planes"):
        assert a["Kmax"] != 8, "this corridor was meant to have blocks of another size"
    else:
        assert a["Kmax"] == 8
    for k in ("f", "g", "f2", "g2"):
        assert a[k] == b[k], (case, k)
    assert a["f"] == a["f2"] and a["g"] == a["g2"]
    assert np.all(np.isfinite(np.frombuffer(bytes.fromhex(a["f"])))) and np.all(np.isfinite(np.frombuffer(bytes.fromhex(a["g"]))))


@pytest.mark.parametrize("case", CLASS_CASES)
def test_class_form_against_the_three_stage_launches(frx, sc, case):
    sname, lname = case.split("-")
    pieces, kappa, obstacles, _ = SHAPES[sname]
    cands = [sc.make_candidate(0, n, n // 4 if n >= 8 else 0, perturb_id=b, obstacles=obstacles) for b, n in enumerate(pieces)]
    prob = frx.Problem(cands, sc.ZHANGJIAJIE, qd_intervals=kappa, **LAYERS[lname])
    try:
        x = prob.initial_guess() + 1e-3 * np.sin(np.arange(prob.NX))
        assert prob.eval_fused() > 0 and prob.eval_geometry() == 1
        f, g = prob.objective(x)
        d = form("default")[case]
        assert f.tobytes().hex() == d["f"] and g.tobytes().hex() == d["g"]       # this process and the fresh child: the same form, the same bits
        prob.set_eval_fused(False)
        try:
            assert prob.eval_geometry() == 0
            f3, g3 = prob.objective(x)
        finally:
            prob.set_eval_fused(True)
        assert np.all(np.isfinite(f)) and np.array_equal(f, f3)
        for b in range(prob.B):
            sl = slice(prob.x_off[b], prob.x_off[b + 1])
            err, scale = np.abs(g[sl] - g3[sl]).max(), max(np.abs(g3[sl]).max(), abs(f3[b]))
            print(f"{case} candidate {b}: gradient differs by {err:.3e}, scale {scale:.3e}")
            assert err <= GRAD_TOL * scale, (case, b)
    finally:
        prob.close()
