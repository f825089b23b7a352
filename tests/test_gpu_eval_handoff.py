"""The hand-off of the penalty partials inside the one-launch evaluation (k_eval_cluster, frx_eval_kernel.hpp; EvalHandoff, frx_kernels.hpp): the members store each
granule with one 16-byte store at its value-major place - granule (value v, piece k) of a candidate with N pieces at word 2 (v N + k) behind its 40 poff words - and the
leader's waves poll them with one coalesced 16-byte load per granule.  Values and the order of every sum are those of the piece-major form (FRX_EVAL_HANDOFF=0), so f and
the gradient are the same BITS; the switch is read once per process, so the forms are compared between child processes started fresh.  The shapes are the ones at which
the transposed index can go wrong: ragged piece counts (N and poff differ per candidate), a last wave-task that is partial and one that is full, a single task, the
smallest candidate, the full wave of 64 pieces, both sample counts (kappa = 16: 3 pieces per wave-task, kappa = 8: 7), one cluster and a second group of eight."""
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

# name: (pieces per candidate, samples per piece - 1).  Pieces per wave-task: 64 // (kappa + 1).
#   kappa = 16 (3 per task): 64 = 21 full tasks + 1 piece, 7 = 2 + 1 piece, 9 = 3 full tasks, 3 = one full task, 2 = one partial task (the smallest candidate)
#   kappa = 8  (7 per task): 64 = 9 full + 1 piece, 14 = 2 full, 10 = 1 + 3 pieces, 7 = one full task, 2 = one partial task
SHAPES = {
    "ragged_k16": ((64, 7, 9, 3, 2), 16),
    "ragged_k8": ((64, 14, 10, 7, 2), 8),
    "one_cluster": ((64,), 16),
    "nine_clusters": ((64, 5, 12, 3, 33, 64, 8, 2, 17), 16),
}

CHILD = r'''
import json, sys
sys.path.insert(0, sys.argv[1])
import numpy as np
from frx_import import frx
from fast_racing_amd import scenario as sc
shapes = json.loads(sys.argv[2])
out = {}
for name, (pieces, kappa) in shapes.items():
    cands = [sc.make_candidate(0, n, n // 4 if n >= 8 else 0, perturb_id=b) for b, n in enumerate(pieces)]
    prob = frx.Problem(cands, sc.ZHANGJIAJIE, qd_intervals=kappa)
    x = prob.initial_guess() + 1e-3 * np.sin(np.arange(prob.NX))
    G = prob.eval_fused()
    f, g = prob.objective(x)
    f2, g2 = prob.objective(x)                                       # the second evaluation on the handle: every granule's address holds the first one's tag
    out[name] = {"G": G, "f": f.tobytes().hex(), "g": g.tobytes().hex(), "again": bool(np.array_equal(f, f2) and np.array_equal(g, g2)), "still": prob.eval_fused()}
    prob.close()
print(json.dumps(out))
'''


def _child(extra_env):
    env = dict(os.environ)
    for k in ("FRX_EVAL_HANDOFF", "FRX_EVAL_FUSED_WT"):
        env.pop(k, None)
    env.update(extra_env)
    p = subprocess.run([sys.executable, "-c", CHILD, ROOT, json.dumps(SHAPES)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=240, env=env)
    assert p.returncode == 0, p.stderr[-2000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


_forms = {}


def form(key):
    """(f, grad f) bits of every shape from one fresh process per form of the switch; computed once, never changed."""
    if key not in _forms:
        _forms[key] = _child({"default": {}, "handoff0": {"FRX_EVAL_HANDOFF": "0"}, "wt": {"FRX_EVAL_FUSED_WT": "1"}}[key])
    return _forms[key]


_handles = {}


def handle(frx, sc, name):
    """One handle per shape in this process (the default form), with its point and its values there."""
    if name not in _handles:
        pieces, kappa = SHAPES[name]
        cands = [sc.make_candidate(0, n, n // 4 if n >= 8 else 0, perturb_id=b) for b, n in enumerate(pieces)]
        prob = frx.Problem(cands, sc.ZHANGJIAJIE, qd_intervals=kappa)
        x = prob.initial_guess() + 1e-3 * np.sin(np.arange(prob.NX))
        f, g = prob.objective(x)
        _handles[name] = (prob, x, f, g)
    return _handles[name]


@pytest.fixture(scope="module", autouse=True)
def _close_handles():
    yield
    for prob, *_ in _handles.values():
        prob.close()
    _handles.clear()


def _geometry(name):
    """Wave-tasks per candidate and the workgroups of a cluster that follow from them: 1 leader + one member per four tasks of the largest candidate."""
    pieces, kappa = SHAPES[name]
    ppw = 64 // (kappa + 1)
    tasks = [(n + ppw - 1) // ppw for n in pieces]
    return ppw, tasks, 1 + (max(tasks) + 3) // 4


@pytest.mark.parametrize("name", list(SHAPES))
def test_the_shapes_are_the_ones_meant(name):
    """The geometry the handle reports is the one the shapes were chosen for: a partial and a full last task, a single task, two clusters' groups."""
    ppw, tasks, G = _geometry(name)
    d = form("default")[name]
    print(f"{name}: {ppw} pieces per wave-task, tasks per candidate {tasks}, {d['G']} workgroups per cluster")
    assert d["G"] == G and d["still"] == G, "the cluster form is not the one in use"
    pieces = SHAPES[name][0]
    if name.startswith("ragged"):
        assert any(n % ppw and n > ppw for n in pieces) and any(n % ppw == 0 and n > ppw for n in pieces)   # last task partial / full, more than one task
        assert any(n == ppw for n in pieces) and any(n < ppw for n in pieces)                                # a single task: full / partial
        assert max(pieces) == 64 and min(pieces) == 2 and len(set(pieces)) == len(pieces)
    if name == "nine_clusters":
        assert len(pieces) == 9
    if name == "one_cluster":
        assert len(pieces) == 1


@pytest.mark.parametrize("name", list(SHAPES))
def test_bits_of_the_two_layouts(name):
    """Value-major granules and 16-byte polls (default) against piece-major granules and 8-byte polls (FRX_EVAL_HANDOFF=0): the same bits, in f and in the gradient."""
    a, b = form("default")[name], form("handoff0")[name]
    assert a["again"] and b["again"]
    assert a["G"] == b["G"] > 0
    assert a["f"] == b["f"], name
    assert a["g"] == b["g"], name
    assert np.all(np.isfinite(np.frombuffer(bytes.fromhex(a["f"]))))


@pytest.mark.parametrize("name", list(SHAPES))
def test_bits_of_the_write_through_path(name):
    """FRX_EVAL_FUSED_WT=1: every granule leaves as two 8-byte write-through stores instead of one plain 16-byte store - the same bits."""
    a, b = form("default")[name], form("wt")[name]
    assert b["again"] and b["G"] == a["G"]
    assert a["f"] == b["f"] and a["g"] == b["g"], name


@pytest.mark.parametrize("name", list(SHAPES))
def test_values_against_the_three_stage_form(frx, sc, name):
    prob, x, f, g = handle(frx, sc, name)
    assert prob.eval_fused() > 0
    d = form("default")[name]
    assert f.tobytes().hex() == d["f"] and g.tobytes().hex() == d["g"]           # this process and the fresh child: the same form, the same bits
    prob.set_eval_fused(False)
    try:
        f3, g3 = prob.objective(x)
    finally:
        prob.set_eval_fused(True)
    assert np.all(np.isfinite(f)) and np.array_equal(f, f3)
    for b in range(prob.B):
        sl = slice(prob.x_off[b], prob.x_off[b + 1])
        err, scale = np.abs(g[sl] - g3[sl]).max(), max(np.abs(g3[sl]).max(), abs(f3[b]))
        print(f"{name} candidate {b}: gradient differs by {err:.3e}, scale {scale:.3e}")
        assert err <= GRAD_TOL * scale, (name, b)


@pytest.mark.parametrize("name", ["ragged_k16", "ragged_k8"])
def test_no_granule_of_an_earlier_evaluation_is_taken(frx, sc, name):
    """Three evaluations at three points on one handle with no synchronisation between the launches, then the same three captured as one graph of three nodes and
    replayed twice: every result equals that of a FRESH handle at that point, bit for bit.  A granule read at an address that still holds an earlier evaluation's
    value under a tag taken for this one's, or a value stored to another granule's place, shows here."""
    prob, x, _, _ = handle(frx, sc, name)
    pieces, kappa = SHAPES[name]
    xs = [x + 2e-3 * (k + 1) * np.cos(np.arange(prob.NX) + k) for k in range(3)]
    want = []
    for v in xs:
        fresh = frx.Problem([sc.make_candidate(0, n, n // 4 if n >= 8 else 0, perturb_id=b) for b, n in enumerate(pieces)], sc.ZHANGJIAJIE, qd_intervals=kappa)
        try:
            assert fresh.eval_fused() > 0
            want.append(fresh.objective(v))
        finally:
            fresh.close()
    assert not np.array_equal(want[0][0], want[2][0])
    H = hip()
    st = Stream()
    xd = [DevBuf(v) for v in xs]
    fd = [DevBuf(np.zeros(prob.B)) for _ in xs]
    gd = [DevBuf(np.zeros(prob.NX)) for _ in xs]
    graph, exe = C.c_void_p(), C.c_void_p()

    def check(what):
        for k in range(3):
            assert np.array_equal(fd[k].get(), want[k][0]) and np.array_equal(gd[k].get(), want[k][1]), (what, k)
            assert H.hipMemcpy(fd[k].ptr, np.zeros(prob.B).ctypes.data, 8 * prob.B, 1) == 0      # (cleared: the next round has to write them again)
            assert H.hipMemcpy(gd[k].ptr, np.zeros(prob.NX).ctypes.data, 8 * prob.NX, 1) == 0
    try:
        for k in range(3):
            prob.objective_device(xd[k].p, fd[k].p, gd[k].p, st.st.value)
        st.sync()
        prob.eval_status()
        check("back to back")
        assert H.hipStreamBeginCapture(st.st, 0) == 0                # hipStreamCaptureModeGlobal
        for k in range(3):
            prob.objective_device(xd[k].p, fd[k].p, gd[k].p, st.st.value)
        assert H.hipStreamEndCapture(st.st, C.byref(graph)) == 0
        assert H.hipGraphInstantiate(C.byref(exe), graph, None, None, 0) == 0
        for replay in range(2):
            assert H.hipGraphLaunch(exe, st.st) == 0
            st.sync()
            prob.eval_status()
            check(f"replay {replay}")
        assert prob.eval_fused() > 0
    finally:
        if exe.value:
            H.hipGraphExecDestroy(exe)
        if graph.value:
            H.hipGraphDestroy(graph)
        for b in xd + fd + gd:
            b.close()
        st.close()
