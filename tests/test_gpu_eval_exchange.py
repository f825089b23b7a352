"""The neighbour exchange of the adjoint solve in the one-launch evaluation (k_eval_cluster; lane_exchange, frx_wave.hpp; pcr_neighbours_reg, frx_kernels.hpp): the
leader's mu = K^-1 wbar (EvalHandoff's transposed form) takes the neighbours k -+ 2^st of its unrolled steps through wave shifts (strides 1, 2) and permlane swaps
(16, 32) instead of shuffles.  Data movement only - no operand and no order of a sum changes - so f and the gradient are the BITS of the forms that keep the
shuffles, FRX_EVAL_HANDOFF=0 FRX_EVAL_EARLY_T=0.  The switches are read once per process, so the forms are compared between child processes started fresh.

Pieces per candidate at kappa = 8: 2, 3, 4, 5, 6, 9, 10, 17, 18, 33, 34, 63, 64 - a solve of N - 1 interior knots takes 0, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 6 steps, every count
from none to six, and the two sides of each power of two are where a lane's `inlo` / `inhi` (has this knot a neighbour 2^st away) change.  The headline geometry
(kappa = 16, a longest candidate of 64 pieces) with 64, 33 and 34 pieces runs the compile-time geometry class.  Each with the soft and with the fixed total time, each
evaluated twice, and once more in the instantiation that carries the cycle stamps (FRX_EVAL_CHAIN=0 launches it for every evaluation; frx_debug_profile_eval_tail for the
one it times), whose six step stamps of the solve must be there and in order."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name: (pieces per candidate, samples per piece - 1, takes the geometry class)
SHAPES = {
    "every_step_count_k8": ((2, 3, 4, 5, 6, 9, 10, 17, 18, 33, 34, 63, 64), 8, 0),
    "headline_geometry": ((64, 33, 34), 16, 1),
}
# the duration layers as tests/test_gpu_parity.py builds them: soft total time (the default), fixed total time
LAYERS = {
    "soft": {},
    "fixed": {"rho": 0.0, "total_t": 9.0, "c2_diffeo": 1},
}
CASES = [f"{s}-{l}" for s in SHAPES for l in LAYERS]
SHUFFLES = {"FRX_EVAL_HANDOFF": "0", "FRX_EVAL_EARLY_T": "0"}
FORMS = {"default": {}, "shuffles": SHUFFLES, "stamped": {"FRX_EVAL_CHAIN": "0"}, "stamped_shuffles": dict(SHUFFLES, FRX_EVAL_CHAIN="0")}

CHILD = r'''
import json, sys
sys.path.insert(0, sys.argv[1])
import numpy as np
from frx_import import frx
from fast_racing_amd import scenario as sc
shapes, layers = json.loads(sys.argv[2]), json.loads(sys.argv[3])
out = {}
for sname, (pieces, kappa, _) in shapes.items():
    for lname, over in layers.items():
        cands = [sc.make_candidate(0, n, n // 4 if n >= 8 else 0, perturb_id=b) for b, n in enumerate(pieces)]
        prob = frx.Problem(cands, sc.ZHANGJIAJIE, qd_intervals=kappa, **over)
        x = prob.initial_guess() + 1e-3 * np.sin(np.arange(prob.NX))
        f, g = prob.objective(x)
        f2, g2 = prob.objective(x)                                   # the second evaluation on the handle
        st = prob.profile_eval_tail(x)                               # the diagnostic: one evaluation of the stamped instantiation
        f3, g3 = prob.objective(x)                                   # and the evaluation behind it
        out[sname + "-" + lname] = {"G": prob.eval_fused(), "geom": prob.eval_geometry(), "f": f.tobytes().hex(), "g": g.tobytes().hex(),
                                    "again": bool(np.array_equal(f, f2) and np.array_equal(g, g2)), "behind": bool(np.array_equal(f, f3) and np.array_equal(g, g3)),
                                    "stamps": [int(v) for v in st]}
        prob.close()
print(json.dumps(out))
'''


def _child(extra_env):
    env = dict(os.environ)
    for k in ("FRX_EVAL_GEOM", "FRX_EVAL_CHAIN", "FRX_EVAL_HANDOFF", "FRX_EVAL_TAIL", "FRX_EVAL_EARLY_T", "FRX_EVAL_ARGPTR", "FRX_EVAL_FRONT", "FRX_EVAL_FUSED", "FRX_EVAL_FUSED_WT"):
        env.pop(k, None)
    env.update(extra_env)
    p = subprocess.run([sys.executable, "-c", CHILD, ROOT, json.dumps(SHAPES), json.dumps(LAYERS)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=240, env=env)
    assert p.returncode == 0, p.stderr[-2000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


_forms = {}


def form(key):
    """(f, grad f) bits of every case from one fresh process per form; computed once, never changed."""
    if key not in _forms:
        _forms[key] = _child(FORMS[key])
    return _forms[key]


def _steps(n):
    """Reduction steps of a candidate of n pieces, as the kernels count them."""
    nst, s = 0, 1
    while s < n - 1:
        nst, s = nst + 1, 2 * s
    return nst


def test_the_shapes_are_the_ones_meant():
    pieces = SHAPES["every_step_count_k8"][0]
    assert sorted(set(_steps(n) for n in pieces)) == [0, 1, 2, 3, 4, 5, 6]
    for st in range(6):                                              # N - 1 = 2^st + 1 is the first size with a neighbour 2^st away; both sides of it are there
        assert (1 << st) + 1 in pieces and (1 << st) + 2 in pieces, st
    assert 63 in pieces and 64 in pieces                             # the last knot with an upper neighbour 32 away, the full wave
    assert [_steps(n) for n in SHAPES["headline_geometry"][0]] == [6, 5, 6]   # under the class's six unrolled steps: all of them, and one short


@pytest.mark.parametrize("case", CASES)
def test_bits_of_the_register_exchange_and_the_shuffles(case):
    """Default against FRX_EVAL_HANDOFF=0 FRX_EVAL_EARLY_T=0: the same bits in f and in the gradient, on both evaluations of a handle."""
    a, b = form("default")[case], form("shuffles")[case]
    assert a["G"] == b["G"] > 0, "the one-launch form is not in use"
    assert a["geom"] == SHAPES[case.split("-")[0]][2], "the geometry class runs where it was meant to, and only there"
    assert a["again"] and b["again"]
    assert a["f"] == b["f"], case
    assert a["g"] == b["g"], case
    assert np.all(np.isfinite(np.frombuffer(bytes.fromhex(a["f"])))) and np.all(np.isfinite(np.frombuffer(bytes.fromhex(a["g"]))))


@pytest.mark.parametrize("case", CASES)
def test_bits_of_the_stamped_instantiation(case):
    """The instantiation with the cycle stamps, launched for every evaluation (FRX_EVAL_CHAIN=0): the register exchange there against the shuffles there and against
    the production instantiation."""
    a, b, c = form("stamped")[case], form("stamped_shuffles")[case], form("default")[case]
    assert a["G"] == b["G"] == c["G"] > 0
    assert a["again"] and b["again"]
    assert a["f"] == b["f"] == c["f"], case
    assert a["g"] == b["g"] == c["g"], case


@pytest.mark.parametrize("key", list(FORMS))
@pytest.mark.parametrize("case", CASES)
def test_the_diagnostic_entry(case, key):
    """frx_debug_profile_eval_tail between two evaluations: the evaluation behind it has the bits of the one in front.  Cluster 0 of the headline handle is a 64-piece
    candidate: its axis wave 1 stamps Hermite adjoint done (74), each of the six steps of the solve (34..39) and wave 0 stamps the barrier behind the knot adjoint (64),
    in this order on the one 100 MHz counter.  Cluster 0 of the other handle has two pieces and no step to stamp."""
    d = form(key)[case]
    assert d["behind"], case
    st = d["stamps"]
    assert len(st) == 80 and st[40] > 0 and st[43] > st[40]
    if case.startswith("headline_geometry"):
        seq = [st[74]] + [st[34 + s] for s in range(6)] + [st[64]]
        print(f"{case} ({key}): 74, 34..39, 64 = {[v - seq[0] for v in seq]} ticks of 10 ns after the first")
        assert all(v > 0 for v in seq), seq
        assert all(p <= q for p, q in zip(seq, seq[1:])), seq
    else:
        assert all(st[34 + s] == 0 for s in range(6)), st[34:40]
