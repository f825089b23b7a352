"""Generates tests/golden/refpin_cases.npz: the REFERENCE's own outputs for every case of
tests/test_reference_pin.py::test_oracle_reproduces_the_reference_cpu_path - its CPU path compiled unmodified against
oracle/eigen_shim (oracle/_ref/libref_gcopter.so) - at the points that test evaluates.  Where that library cannot be
built (no reference tree), the test pins the oracle to these stored outputs instead.  Run from the repo root after build():
    python tests/golden/make_refpin.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from frx_import import frx  # noqa: E402,F401
from fast_racing_amd import scenario as sc  # noqa: E402
from oracle import binding as ob  # noqa: E402
from test_reference_pin import CASES, reference_outputs  # noqa: E402


def main():
    if ob.ref_gcopter() is None:
        raise SystemExit("oracle/_ref/libref_gcopter.so not built: nothing to record")
    out = {}
    for i, (sid, N, gates, kappa, obst, over) in enumerate(CASES):
        cand = sc.make_candidate(sid, N, gates, obstacles=obst)
        o = ob.Oracle(cand, sc.ZHANGJIAJIE, qd_intervals=kappa, **over)
        r = ob.Reference(cand, sc.ZHANGJIAJIE, override_vs=True, qd_intervals=kappa, **over)
        for k, v in reference_outputs(o, r).items():
            out[f"{i}_{k}"] = v
    path = os.path.join(ROOT, "tests", "golden", "refpin_cases.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(CASES)} cases, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
