"""Launches under the settings of the one-launch evaluation's switches that no other test launches: by value (FRX_EVAL_ARGPTR=0), f and `done` behind the kernel's last
barrier (FRX_EVAL_TAIL=0), staged durations by value, the stamped hand-off form in production (FRX_EVAL_CHAIN=0) and the run-time form on a handle of the geometry
class (FRX_EVAL_GEOM=0).  The switches are read once per process, so every setting runs in a child process started fresh.  The handle is of pieces (64, 2) at
kappa = 16: the geometry class; more than 64 KB of dynamic LDS per workgroup, so a form whose limit nobody raised fails at its launch; a full and a one-piece
candidate.  What a child shows: under its setting the launch is accepted, the cluster form stays in use, f equals the three stage launches' bit for bit and the
gradient is within their bound.  WHICH instantiation ran is not observed here (the library reports only the class flag, which is asserted): that a setting maps to
its form is tests/test_launch_forms_cpu.py's, on the function the launcher asks.

And the corridor-cell entry called three times.  That a kernel's limit only grows is NOT checked here - frx_dilate_batch fixes the candidate capacity, so every
call through it has the same LDS need - but on the table itself, with a recording setter, in tests/test_launch_forms_cpu.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dilate_states as ds  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRAD_TOL = 1e-10           # one launch against three stage launches, per candidate: |g1 - g3|max <= 1e-10 max(|g3|max, |f3|) - the bound of tests/test_gpu_parity.py for these two forms
PIECES, KAPPA = (64, 2), 16

# setting: (environment, 1 when the handle launches the geometry class)
SETTINGS = {
    "default": ({}, 1),
    "argptr0": ({"FRX_EVAL_ARGPTR": "0"}, 0),
    "tail0": ({"FRX_EVAL_TAIL": "0"}, 0),
    "argptr0_early0": ({"FRX_EVAL_ARGPTR": "0", "FRX_EVAL_EARLY_T": "0"}, 0),
    "chain0": ({"FRX_EVAL_CHAIN": "0"}, 1),
    "geom0": ({"FRX_EVAL_GEOM": "0"}, 0),
}

CHILD = r'''
import json, sys
sys.path.insert(0, sys.argv[1])
import numpy as np
from frx_import import frx
from fast_racing_amd import scenario as sc
pieces, kappa = json.loads(sys.argv[2])
cands = [sc.make_candidate(0, n, n // 4 if n >= 8 else 0, perturb_id=b) for b, n in enumerate(pieces)]
prob = frx.Problem(cands, sc.ZHANGJIAJIE, qd_intervals=kappa)
x = prob.initial_guess() + 1e-3 * np.sin(np.arange(prob.NX))
out = {"G": prob.eval_fused(), "class": prob.eval_geometry(), "x_off": [int(v) for v in prob.x_off]}
f, g = prob.objective(x)
f2, g2 = prob.objective(x)                                           # both evaluations succeed (an expired wait or a refused launch raises)
out["still"] = prob.eval_fused()
prob.set_eval_fused(False)
f3, g3 = prob.objective(x)
out.update(f=f.tobytes().hex(), g=g.tobytes().hex(), again=bool(np.array_equal(f, f2) and np.array_equal(g, g2)), f3=f3.tobytes().hex(), g3=g3.tobytes().hex())
prob.close()
print(json.dumps(out))
'''


@pytest.mark.parametrize("name", list(SETTINGS))
def test_rung(name):
    extra, is_class = SETTINGS[name]
    env = {k: v for k, v in os.environ.items() if not k.startswith("FRX_EVAL_")}
    env.update(extra)
    p = subprocess.run([sys.executable, "-c", CHILD, ROOT, json.dumps([PIECES, KAPPA])], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120, env=env)
    assert p.returncode == 0, p.stderr[-2000:]
    r = json.loads(p.stdout.strip().splitlines()[-1])
    ppw = 64 // (KAPPA + 1)
    G = 1 + ((max(PIECES) + ppw - 1) // ppw + 3) // 4
    assert r["G"] == G and r["still"] == G, "the cluster form is not (or no longer) the one in use"
    assert r["class"] == is_class
    assert r["again"]
    f, g, f3, g3 = (np.frombuffer(bytes.fromhex(r[k])) for k in ("f", "g", "f3", "g3"))
    assert np.all(np.isfinite(f)) and np.array_equal(f, f3)
    for b in range(len(PIECES)):
        sl = slice(r["x_off"][b], r["x_off"][b + 1])
        err, scale = np.abs(g[sl] - g3[sl]).max(), max(np.abs(g3[sl]).max(), abs(f3[b]))
        print(f"{name} candidate {b}: gradient differs by {err:.3e}, scale {scale:.3e}")
        assert err <= GRAD_TOL * scale, (name, b)


def test_the_cell_entry_repeats_with_its_limit_already_held(frx):
    """One segment, a cloud of a few hundred points, the entry's plane capacity large, exact, large: the second and third launch find k_dilate's need (that of 4096
    candidate points, whatever the plane capacity) already held and make no call for it; every call succeeds and gives the first one's cell, bit for bit."""
    st = ds.size_state(257)
    assert 200 <= len(st.obs) <= 999 and st.K < 512
    cell = {cap: frx.dilate_batch(st.p1[None], st.p2[None], st.bbox, st.obs, cap_planes=cap)[0] for cap in (512, st.K)}
    again = frx.dilate_batch(st.p1[None], st.p2[None], st.bbox, st.obs, cap_planes=512)[0]
    for a, b in zip(cell[512], again):
        assert np.array_equal(a, b)
    for a, b in zip(cell[512], cell[st.K]):
        assert np.array_equal(a, b)
    assert cell[512][0].shape[1] == st.K
