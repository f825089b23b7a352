#!/usr/bin/env python3
"""Throughput of the exact gate passage certificate on the device (frx_trajectory_gates, csrc/frx_gates_kernel.hpp) at two shapes: 32 candidates x 64 pieces x
16 gates (a planner's batch with every gate of the course) and 4096 x 64 x 3 (a Monte-Carlo batch).  The trajectories are the initial guesses of 32 scenarios,
repeated; each candidate's gates are its scenario's own, framed along the bisector of the polyline with half extents 1 m x 0.75 m.

Per shape: the _device form timed with HIP events around `--reps` back-to-back launches on one stream after a warm-up launch (the launch interval), and the
blocking form with a host clock (upload, launch, download, flags).  There is no target: the file records what the kernel does.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="32x64x16,4096x64x3", help="candidates x pieces x gates per candidate, comma separated")
ap.add_argument("--kappa", type=int, default=16)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gates_throughput.json"))
args = ap.parse_args()

import numpy as np  # noqa: E402
import torch  # noqa: E402

from frx_import import frx  # noqa: E402
from fast_racing_amd import scenario as sc  # noqa: E402

torch.cuda.init()                         # torch's HIP runtime first, then the library's (the order bench.py keeps)
if frx.lib().frx_device_count() < 1:
    raise SystemExit("gates_throughput.py needs a HIP device")

BOX = np.concatenate([np.vstack([np.eye(3), np.diag([2.0, 2.0, 4.0])]), np.vstack([-np.eye(3), np.diag([-2.0, -2.0, 0.0])])], axis=1)


def frames(cand, half_u=1.0, half_v=0.75):
    """gate records of a scenario candidate: the normal along the bisector of the polyline start -> gates -> goal, ev the vertical made orthogonal to it"""
    poly = np.vstack([cand.ini_state[:, 0], cand.gates, cand.fin_state[:, 0]])
    out = []
    for k, c in enumerate(cand.gates):
        d0, d1 = poly[k + 1] - poly[k], poly[k + 2] - poly[k + 1]
        n = d0 / np.linalg.norm(d0) + d1 / np.linalg.norm(d1)
        n /= np.linalg.norm(n)
        ev = np.array([0.0, 0.0, 1.0]) - n[2] * n
        ev /= np.linalg.norm(ev)
        out.append(np.concatenate([c, half_u * np.cross(ev, n), half_v * ev]))
    return np.array(out)


stream = torch.cuda.current_stream().cuda_stream
rows = []
for shape in args.shapes.split(","):
    B, N, G = (int(v) for v in shape.split("x"))
    n_src = min(B, 32)
    src = [sc.make_candidate(s, N, G) for s in range(n_src)]
    plan = frx.Problem(src, sc.ZHANGJIAJIE, qd_intervals=args.kappa)
    T0, C0 = plan.forward(plan.initial_guess())
    plan.close()
    idx = np.arange(B) % n_src
    T = np.ascontiguousarray(np.asarray(T0).reshape(n_src, N)[idx]).reshape(-1)
    Cf = np.ascontiguousarray(np.asarray(C0).reshape(n_src, N * 18)[idx]).reshape(-1)
    gates = np.ascontiguousarray(np.array([frames(c) for c in src])[idx]).reshape(-1, 9)
    gate_off = (np.arange(B + 1) * G).astype(np.int32)
    prob = frx.PenaltyProblem(sc.ZHANGJIAJIE, [N] * B, [0] * (B * N), [BOX], qd_intervals=args.kappa)
    d_T, d_C, d_g, d_off = (torch.from_numpy(a).cuda() for a in (T, Cf, gates.reshape(-1), gate_off))
    d_out = torch.zeros(B * G * 10, dtype=torch.float64, device="cuda")

    def launch():
        prob.trajectory_gates_device(d_T.data_ptr(), d_C.data_ptr(), B * G, d_off.data_ptr(), d_g.data_ptr(), d_out.data_ptr(), stream)

    launch()                                                             # warm-up
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.reps):
        launch()
    e1.record()
    torch.cuda.synchronize()
    row = dict(candidates=B, pieces_per_candidate=N, gates_per_candidate=G, device_launch_ms=e0.elapsed_time(e1) / args.reps)
    row["ns_per_piece_gate"] = row["device_launch_ms"] * 1e6 / (B * N * G)
    dev = d_out.cpu().numpy().reshape(-1, 10)
    prob.trajectory_gates(T, Cf, gates, gate_off)
    t0 = time.perf_counter()
    got = prob.trajectory_gates(T, Cf, gates, gate_off)
    row["blocking_call_ms"] = (time.perf_counter() - t0) * 1e3
    assert np.array_equal(got["gate"], dev, equal_nan=True)
    row["gates_crossed"] = int((got["n_cross"] > 0).sum())
    row["gates_passed"] = int((got["n_pass"] > 0).sum())
    row["candidates_flagged"] = int((got["flags"] != 0).sum())
    rows.append(row)
    print(json.dumps(row), flush=True)
    prob.close()
res = dict(what="frx_trajectory_gates: the _device form's launch interval and the blocking call", reps=args.reps, rows=rows)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(res, f, indent=1)
