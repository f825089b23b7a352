"""The production instantiation of the one-launch evaluation (k_eval_cluster<.., CH>, frx_eval_kernel.hpp; EvalChain, frx_kernels.hpp): no cycle stamps compiled in, and
what the stretches behind the forward map read from the argument block loaded once and held in scalar registers.  The expressions and the order of every sum are those of
the form with the stamps (FRX_EVAL_CHAIN=0, which is also what the diagnostics launch), so f and the gradient are the same BITS; the switch is read once per process, so
the forms are compared between child processes started fresh.  Shapes: one waypoint and one active knot with a single coarse interval in the merge loop, the first lane
shift, ragged candidates with partial and full wave-tasks at both sample counts, a second group of eight clusters.  Both duration layers - soft total time, and fixed
total time (rho = 0, where the tail reads `soft`, `sumT` and `c2` from the argument block) with both maps tau -> T.  Around frx_debug_profile_eval_cluster: the handle
launches the stamped instantiation with an argument block of its own for that one evaluation and nothing else changes - not the next evaluation, not a graph captured
before."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_eval_tail import DevBuf, Stream, hip  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRAD_TOL = 1e-10           # one launch against three stage launches, per candidate: |g1 - g3|max <= 1e-10 max(|g3|max, |f3|) - the bound of tests/test_gpu_parity.py for these two forms

# name: (pieces per candidate, samples per piece - 1)
SHAPES = {
    "one_waypoint": ((2,), 8),
    "first_lane_shift": ((3,), 16),
    "ragged_k16": ((64, 7, 9, 3, 2), 16),
    "ragged_k8": ((64, 14, 10, 7, 2), 8),
    "nine_clusters": ((64, 5, 12, 3, 33, 64, 8, 2, 17), 16),
}
# the duration layers as tests/test_gpu_parity.py builds them: soft total time (the default), fixed total time with the C2 map and with the exponential one
LAYERS = {
    "soft": {},
    "fixed": {"rho": 0.0, "total_t": 9.0, "c2_diffeo": 1},
    "fixed_exp": {"rho": 0.0, "total_t": 9.0, "c2_diffeo": 0},
}
CASES = [f"{s}-{l}" for s in SHAPES for l in LAYERS]
# thread 0 of cluster 0's leader, in program order on one shader clock: entry, the forward map's stamps, the adjoint's
ORDERED_SHADER = (49, 0, 2, 5, 6, 16, 17, 22, 23, 24)
# the leader's 100 MHz stamps: entry, forward map done, out of the adjoint, end
ORDERED_WALL = (40, 41, 42, 43)

CHILD = r'''
import json, sys
sys.path.insert(0, sys.argv[1])
import numpy as np
from frx_import import frx
from fast_racing_amd import scenario as sc
shapes, layers = json.loads(sys.argv[2]), json.loads(sys.argv[3])
out = {}
for sname, (pieces, kappa) in shapes.items():
    for lname, over in layers.items():
        cands = [sc.make_candidate(0, n, n // 4 if n >= 8 else 0, perturb_id=b) for b, n in enumerate(pieces)]
        prob = frx.Problem(cands, sc.ZHANGJIAJIE, qd_intervals=kappa, **over)
        x = prob.initial_guess() + 1e-3 * np.sin(np.arange(prob.NX))
        G = prob.eval_fused()
        f, g = prob.objective(x)
        f2, g2 = prob.objective(x)                                   # the second evaluation on the handle
        st = prob.profile_eval_tail(x)                               # the diagnostic: one evaluation of the stamped instantiation
        f3, g3 = prob.objective(x)                                   # and the evaluation behind it
        out[sname + "-" + lname] = {"G": G, "f": f.tobytes().hex(), "g": g.tobytes().hex(), "again": bool(np.array_equal(f, f2) and np.array_equal(g, g2)),
                                    "behind": bool(np.array_equal(f, f3) and np.array_equal(g, g3)), "stamps": [int(v) for v in st], "still": prob.eval_fused()}
        prob.close()
print(json.dumps(out))
'''


def _child(extra_env):
    env = dict(os.environ)
    for k in ("FRX_EVAL_CHAIN", "FRX_EVAL_HANDOFF", "FRX_EVAL_TAIL", "FRX_EVAL_EARLY_T", "FRX_EVAL_ARGPTR", "FRX_EVAL_FUSED_WT"):
        env.pop(k, None)
    env.update(extra_env)
    p = subprocess.run([sys.executable, "-c", CHILD, ROOT, json.dumps(SHAPES), json.dumps(LAYERS)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=240, env=env)
    assert p.returncode == 0, p.stderr[-2000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


_forms = {}


def form(key):
    """(f, grad f) bits of every case from one fresh process per form of the switch; computed once, never changed."""
    if key not in _forms:
        _forms[key] = _child({"default": {}, "chain0": {"FRX_EVAL_CHAIN": "0"}}[key])
    return _forms[key]


def _problem(frx, sc, case):
    sname, lname = case.split("-")
    pieces, kappa = SHAPES[sname]
    cands = [sc.make_candidate(0, n, n // 4 if n >= 8 else 0, perturb_id=b) for b, n in enumerate(pieces)]
    prob = frx.Problem(cands, sc.ZHANGJIAJIE, qd_intervals=kappa, **LAYERS[lname])
    return prob, prob.initial_guess() + 1e-3 * np.sin(np.arange(prob.NX))


@pytest.mark.parametrize("case", CASES)
def test_bits_of_the_two_forms(case):
    """The production instantiation (default) against the one with the stamps and the argument loads at their uses (FRX_EVAL_CHAIN=0): the same bits in f and in the
    gradient, on the first evaluation and on the second one on the same handle."""
    a, b = form("default")[case], form("chain0")[case]
    assert a["G"] == b["G"] > 0 and a["still"] == a["G"] and b["still"] == b["G"], "the cluster form is not the one in use"
    assert a["again"] and b["again"]
    assert a["f"] == b["f"], case
    assert a["g"] == b["g"], case
    assert np.all(np.isfinite(np.frombuffer(bytes.fromhex(a["f"])))) and np.all(np.isfinite(np.frombuffer(bytes.fromhex(a["g"]))))


@pytest.mark.parametrize("key", ["default", "chain0"])
@pytest.mark.parametrize("case", CASES)
def test_the_diagnostic_leaves_the_handle_as_it_was(case, key):
    """An evaluation, frx_debug_profile_eval_tail, another evaluation: the stamps are there and in order, and the evaluation behind the diagnostic has the bits of the
    one in front of it."""
    d = form(key)[case]
    st = d["stamps"]
    for seq in (ORDERED_SHADER, ORDERED_WALL):
        v = [st[i] for i in seq]
        print(f"{case} ({key}): stamps {seq} = {[x - v[0] for x in v]} after the first")
        assert all(x > 0 for x in v), (case, seq, v)
        assert all(a <= b for a, b in zip(v, v[1:])), (case, seq, v)
    assert st[43] > st[40] and st[24] > st[49]
    assert d["behind"], case


@pytest.mark.parametrize("case", CASES)
def test_values_against_the_three_stage_form(frx, sc, case):
    prob, x = _problem(frx, sc, case)
    try:
        assert prob.eval_fused() > 0
        f, g = prob.objective(x)
        d = form("default")[case]
        assert f.tobytes().hex() == d["f"] and g.tobytes().hex() == d["g"]       # this process and the fresh child: the same form, the same bits
        prob.set_eval_fused(False)
        try:
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


@pytest.mark.parametrize("case", ["ragged_k16-soft", "ragged_k8-fixed"])
def test_a_graph_captured_before_the_diagnostic_replays_after_it(frx, sc, case):
    """The evaluation is captured, the diagnostic runs (it launches the other instantiation with the other argument block), the graph is replayed: the bits of the
    evaluation in front of everything.  The captured node points at the production arguments, which no call touches after create."""
    prob, x = _problem(frx, sc, case)
    H = hip()
    st = Stream()
    xd, fd, gd = DevBuf(x), DevBuf(np.zeros(prob.B)), DevBuf(np.zeros(prob.NX))
    graph, exe = C.c_void_p(), C.c_void_p()
    try:
        f0, g0 = prob.objective(x)
        assert H.hipStreamBeginCapture(st.st, 0) == 0                # hipStreamCaptureModeGlobal
        prob.objective_device(xd.p, fd.p, gd.p, st.st.value)
        assert H.hipStreamEndCapture(st.st, C.byref(graph)) == 0
        assert H.hipGraphInstantiate(C.byref(exe), graph, None, None, 0) == 0
        assert H.hipGraphLaunch(exe, st.st) == 0
        st.sync()
        prob.eval_status()
        assert np.array_equal(fd.get(), f0) and np.array_equal(gd.get(), g0)
        stamps = prob.profile_eval_cluster(x)
        assert stamps[40] > 0 and stamps[43] > stamps[40]
        for replay in range(2):
            assert H.hipMemcpy(fd.ptr, np.zeros(prob.B).ctypes.data, 8 * prob.B, 1) == 0         # (cleared: the replay has to write them again)
            assert H.hipMemcpy(gd.ptr, np.zeros(prob.NX).ctypes.data, 8 * prob.NX, 1) == 0
            assert H.hipGraphLaunch(exe, st.st) == 0
            st.sync()
            prob.eval_status()
            assert np.array_equal(fd.get(), f0) and np.array_equal(gd.get(), g0), (case, replay)
        f1, g1 = prob.objective(x)
        assert np.array_equal(f1, f0) and np.array_equal(g1, g0)
        assert prob.eval_fused() > 0
    finally:
        if exe.value:
            H.hipGraphExecDestroy(exe)
        if graph.value:
            H.hipGraphDestroy(graph)
        for b in (xd, fd, gd):
            b.close()
        st.close()
        prob.close()
