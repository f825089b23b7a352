"""The two-trip front of the one-launch evaluation (k_eval_cluster<.., FR>, frx_eval_kernel.hpp): a workgroup reads its candidate's front record and the argument block's
leading lines, then issues every operand load of the front as one group, instead of walking the offset tables.  Only integers and the order of loads differ from the
front that walks the tables (FRX_EVAL_FRONT=0), so f and the gradient are the same BITS; the switch is read once per process, so the two fronts are compared between
child processes started fresh, and Problem.eval_front() says which one a handle launches.

Shapes: the headline geometry (64,); ragged candidates; nine candidates - a second group of eight blocks, so that a cluster's index differs from its position in the
group; (3,) and (2,) alone - the run-time form with one reduction step or none; kappa = 8 - a run-time geometry; a corridor with obstacle planes, whose blocks are not
8 half-spaces.  Each with the soft and with the fixed total time."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name: (pieces per candidate, samples per piece - 1, corridor with obstacle planes)
SHAPES = {
    "headline": ((64,), 16, False),
    "ragged": ((64, 7, 9, 3, 2), 16, False),
    "nine_clusters": ((64, 5, 12, 3, 33, 64, 8, 2, 17), 16, False),
    "three_pieces": ((3,), 16, False),
    "two_pieces": ((2,), 16, False),
    "kappa8": ((64, 14, 10, 7, 2), 8, False),
    "obstacle_planes": ((64, 7), 16, True),
}
# the duration layers as tests/test_gpu_parity.py builds them: soft total time (the default), fixed total time
LAYERS = {
    "soft": {},
    "fixed": {"rho": 0.0, "total_t": 9.0, "c2_diffeo": 1},
}
CASES = [f"{s}-{l}" for s in SHAPES for l in LAYERS]

CHILD = r'''
import json, sys
sys.path.insert(0, sys.argv[1])
import numpy as np
from frx_import import frx
from fast_racing_amd import scenario as sc
shapes, layers = json.loads(sys.argv[2]), json.loads(sys.argv[3])
out = {}
for sname, (pieces, kappa, obstacles) in shapes.items():
    for lname, over in layers.items():
        cands = [sc.make_candidate(0, n, n // 4 if n >= 8 else 0, perturb_id=b, obstacles=bool(obstacles)) for b, n in enumerate(pieces)]
        prob = frx.Problem(cands, sc.ZHANGJIAJIE, qd_intervals=kappa, **over)
        x = prob.initial_guess() + 1e-3 * np.sin(np.arange(prob.NX))
        f, g = prob.objective(x)
        f2, g2 = prob.objective(x)                                   # the second evaluation on the handle
        out[sname + "-" + lname] = {"G": prob.eval_fused(), "front": prob.eval_front(), "Kmax": prob.Kmax, "f": f.tobytes().hex(), "g": g.tobytes().hex(),
                                    "f2": f2.tobytes().hex(), "g2": g2.tobytes().hex()}
        prob.close()
print(json.dumps(out))
'''


def _child(extra_env):
    env = dict(os.environ)
    for k in ("FRX_EVAL_FRONT", "FRX_EVAL_GEOM", "FRX_EVAL_CHAIN", "FRX_EVAL_HANDOFF", "FRX_EVAL_TAIL", "FRX_EVAL_EARLY_T", "FRX_EVAL_ARGPTR", "FRX_EVAL_FUSED", "FRX_EVAL_FUSED_WT"):
        env.pop(k, None)
    env.update(extra_env)
    p = subprocess.run([sys.executable, "-c", CHILD, ROOT, json.dumps(SHAPES), json.dumps(LAYERS)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=240, env=env)
    assert p.returncode == 0, p.stderr[-2000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


_forms = {}


def form(key):
    """(f, grad f) bits of every case from one fresh process per value of the switch; computed once, never changed."""
    if key not in _forms:
        _forms[key] = _child({"default": {}, "front0": {"FRX_EVAL_FRONT": "0"}}[key])
    return _forms[key]


@pytest.mark.parametrize("case", CASES)
def test_bits_of_the_two_fronts(case):
    """Default against FRX_EVAL_FRONT=0: the one-launch form in both, the query 1 and 0, the same bits in f and in the gradient on the first and on the second evaluation
    of a handle."""
    a, b = form("default")[case], form("front0")[case]
    assert a["G"] > 0 and b["G"] > 0 and a["G"] == b["G"], "the one-launch form is not in use"
    assert a["front"] == 1 and b["front"] == 0, (case, a["front"], b["front"])
    if case.startswith("obstacle_planes"):
        assert a["Kmax"] != 8, "this corridor was meant to have blocks of another size"
    for k in ("f", "g", "f2", "g2"):
        assert a[k] == b[k], (case, k)
    assert a["f"] == a["f2"] and a["g"] == a["g2"]
    assert np.all(np.isfinite(np.frombuffer(bytes.fromhex(a["f"])))) and np.all(np.isfinite(np.frombuffer(bytes.fromhex(a["g"]))))


@pytest.mark.parametrize("case", CASES)
def test_stamped_evaluation_then_a_plain_one(frx, sc, case):
    """In this process: one stamped evaluation (the diagnostics' instantiation, with its own argument block) followed by a plain one gives the child's bits again."""
    sname, lname = case.split("-")
    pieces, kappa, obstacles = SHAPES[sname]
    cands = [sc.make_candidate(0, n, n // 4 if n >= 8 else 0, perturb_id=b, obstacles=obstacles) for b, n in enumerate(pieces)]
    prob = frx.Problem(cands, sc.ZHANGJIAJIE, qd_intervals=kappa, **LAYERS[lname])
    try:
        x = prob.initial_guess() + 1e-3 * np.sin(np.arange(prob.NX))
        assert prob.eval_fused() > 0 and prob.eval_front() == 1
        st = prob.profile_eval_cluster(x)
        assert st[40] > 0 and st[43] > st[40]                        # the leader's entry and end
        assert st[40] <= st[32] <= st[33] <= st[50]                  # entry, tau issued, tau landed, durations formed
        f, g = prob.objective(x)
        d = form("default")[case]
        assert f.tobytes().hex() == d["f"] and g.tobytes().hex() == d["g"]
    finally:
        prob.close()
