"""The leader's adjoint of the one-launch evaluation with its operands in front of the poll (k_eval_cluster<.., ADJ>, backward_knot_wsp64 with EvalHandoff<.., AJ>): the
adjoint's top takes the offsets, the lane's waypoint entries and the tail states from what the workgroup's front already holds instead of walking the offset tables, and
an axis lane requests its waypoint-layer operands - eight clamped reads each of xi and of the three vertex coordinates, the forward map's four sums, the division and the
three scale factors - next to the multipliers, in front of the poll for the penalty partials.  No floating-point expression, operand or order differs from the form
before (FRX_EVAL_ADJOINT=0), so f and the gradient are the same BITS; the switch is read once per process, so the two are compared between child processes started
fresh, and Problem.eval_adjoint() says which one a handle launches.

Shapes: the seven of tests/test_gpu_eval_front.py, and two built by hand for the operand reads -
  few_vertices   waypoint polytopes of 2 and of 3 vertices: the clamped operand index min(sub + 2 j, nv - 2) is 0 (and 0 or 1) for all eight held operands;
  big_v          more than 17 vertices per polytope (33 pieces: with 64 the tripled polytopes no longer fit the one-launch form's LDS): the remainder loop behind the
                 eight held operands runs;
each with the soft and with the fixed total time."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name: (pieces per candidate, samples per piece - 1, corridor with obstacle planes, what is done to the waypoint polytopes by hand)
SHAPES = {
    "headline": ((64,), 16, False, ""),
    "ragged": ((64, 7, 9, 3, 2), 16, False, ""),
    "nine_clusters": ((64, 5, 12, 3, 33, 64, 8, 2, 17), 16, False, ""),
    "three_pieces": ((3,), 16, False, ""),
    "two_pieces": ((2,), 16, False, ""),
    "kappa8": ((64, 14, 10, 7, 2), 8, False, ""),
    "obstacle_planes": ((64, 7), 16, True, ""),
    "few_vertices": ((9, 5), 16, False, "few"),
    "big_v": ((33, 6), 16, False, "dup"),
}
LAYERS = {
    "soft": {},
    "fixed": {"rho": 0.0, "total_t": 9.0, "c2_diffeo": 1},
}
CASES = [f"{s}-{l}" for s in SHAPES for l in LAYERS]

# (shared by the children and by the stamped test below: the same candidates and the same x in every process)
BUILD = r'''
import numpy as np
def build_case(frx, sc, pieces, kappa, obstacles, mod, over):
    cands = [sc.make_candidate(0, n, n // 4 if n >= 8 else 0, perturb_id=b, obstacles=bool(obstacles)) for b, n in enumerate(pieces)]
    if mod:
        c = cands[0]
        for w, j in enumerate(range(1, len(c.v_polys), 2)):          # the overlaps: the waypoint polytopes of a corridor with one piece per cell
            v = c.v_polys[j]
            if mod == "few": c.v_polys[j] = v[:, :2 + (w & 1)].copy()            # a segment, a triangle, a segment, ...
            else: c.v_polys[j] = np.concatenate([v, v[:, 1:], v[:, 1:]], axis=1)   # every vertex but the first three times: 3 nv - 2 vertices
    prob = frx.Problem(cands, sc.ZHANGJIAJIE, qd_intervals=kappa, **over)
    x = 0.5 + 0.3 * np.sin(0.7 * np.arange(prob.NX)) if mod else prob.initial_guess() + 1e-3 * np.sin(np.arange(prob.NX))
    return prob, x, [int(v.shape[1]) for v in cands[0].v_polys[1::2]]
'''

CHILD = BUILD + r'''
import json, sys
sys.path.insert(0, sys.argv[1])
from frx_import import frx
from fast_racing_amd import scenario as sc
shapes, layers = json.loads(sys.argv[2]), json.loads(sys.argv[3])
out = {}
for sname, (pieces, kappa, obstacles, mod) in shapes.items():
    for lname, over in layers.items():
        prob, x, nv = build_case(frx, sc, pieces, kappa, obstacles, mod, over)
        f, g = prob.objective(x)
        f2, g2 = prob.objective(x)                                   # the second evaluation on the handle
        out[sname + "-" + lname] = {"G": prob.eval_fused(), "front": prob.eval_front(), "prelude": prob.eval_prelude(), "adjoint": prob.eval_adjoint(),
                                    "f": f.tobytes().hex(), "g": g.tobytes().hex(), "f2": f2.tobytes().hex(), "g2": g2.tobytes().hex(), "nv_min": min(nv), "nv_max": max(nv)}
        prob.close()
print(json.dumps(out))
'''


def _child(extra_env):
    env = dict(os.environ)
    for k in ("FRX_EVAL_ADJOINT", "FRX_EVAL_PRELUDE", "FRX_EVAL_FRONT", "FRX_EVAL_GEOM", "FRX_EVAL_CHAIN", "FRX_EVAL_HANDOFF", "FRX_EVAL_TAIL", "FRX_EVAL_EARLY_T", "FRX_EVAL_ARGPTR",
              "FRX_EVAL_FUSED", "FRX_EVAL_FUSED_WT"):
        env.pop(k, None)
    env.update(extra_env)
    p = subprocess.run([sys.executable, "-c", CHILD, ROOT, json.dumps(SHAPES), json.dumps(LAYERS)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300, env=env)
    assert p.returncode == 0, p.stderr[-2000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


_forms = {}


def form(key):
    """(f, grad f) bits of every case from one fresh process per value of the switch; computed once, never changed."""
    if key not in _forms:
        _forms[key] = _child({"default": {}, "adjoint0": {"FRX_EVAL_ADJOINT": "0"}}[key])
    return _forms[key]


@pytest.mark.parametrize("case", CASES)
def test_bits_of_the_two_adjoints(case):
    """Default against FRX_EVAL_ADJOINT=0: the one-launch form with the two-trip front and the shortened prelude in both, the query 1 and 0, the same bits in f and in the
    gradient on the first and on the second evaluation of a handle, every value finite; the hand-built shapes have the vertex counts they were meant to have."""
    a, b = form("default")[case], form("adjoint0")[case]
    assert a["G"] > 0 and b["G"] > 0 and a["G"] == b["G"], "the one-launch form is not in use"
    assert a["front"] == 1 and b["front"] == 1 and a["prelude"] == 1 and b["prelude"] == 1
    assert a["adjoint"] == 1 and b["adjoint"] == 0, (case, a["adjoint"], b["adjoint"])
    if case.startswith("few_vertices"):
        assert (a["nv_min"], a["nv_max"]) == (2, 3), (a["nv_min"], a["nv_max"])
    if case.startswith("big_v"):
        assert a["nv_min"] > 17, a["nv_min"]                          # (eight operands per lane of a pair hold vertices 1..16)
    for k in ("f", "g", "f2", "g2"):
        assert a[k] == b[k], (case, k)
    assert a["f"] == a["f2"] and a["g"] == a["g2"]
    assert np.all(np.isfinite(np.frombuffer(bytes.fromhex(a["f"])))) and np.all(np.isfinite(np.frombuffer(bytes.fromhex(a["g"]))))


@pytest.mark.parametrize("case", ["headline-soft", "ragged-fixed", "few_vertices-soft", "big_v-soft"])
def test_stamped_evaluation_then_a_plain_one(frx, sc, case):
    """In this process: one stamped evaluation (the diagnostics' instantiation of the same adjoint) followed by a plain one.  The new stamp - 77, axis wave 1 has
    requested its waypoint-layer operands - lies between the leader's entry and that wave's entry into its poll, the stamps that were there stay monotone along the wave,
    and the plain evaluation gives the child's bits."""
    sname, lname = case.split("-")
    pieces, kappa, obstacles, mod = SHAPES[sname]
    ns = {}
    exec(BUILD, ns)
    prob, x, _ = ns["build_case"](frx, sc, pieces, kappa, obstacles, mod, LAYERS[lname])
    try:
        assert prob.eval_fused() > 0 and prob.eval_adjoint() == 1
        st = prob.profile_eval_tail(x)
        N = int(prob.piece_off[1] - prob.piece_off[0])
        nst = int(np.ceil(np.log2(N - 1))) if N > 2 else 0             # steps of candidate 0's solve
        chains = {
            "axis wave 1": [40, 77, 72, 73, 74] + [34 + s for s in range(nst)] + [64],      # (64: wave 0 behind the barrier that axis wave 1 reaches behind its solve)
            "wave 0": [40, 41, 70, 71, 64, 65, 43],
        }
        for name, slots in chains.items():
            v = [int(st[i]) for i in slots]
            assert all(t > 0 for t in v), (name, dict(zip(slots, v)))
            assert all(a <= b for a, b in zip(v, v[1:])), (name, dict(zip(slots, v)))
        f, g = prob.objective(x)
        d = form("default")[case]
        assert f.tobytes().hex() == d["f"] and g.tobytes().hex() == d["g"]
    finally:
        prob.close()
