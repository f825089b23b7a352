#!/usr/bin/env python3
"""Throughput of the exact corridor containment certificate on the device (frx_trajectory_contain, csrc/frx_contain_kernel.hpp) at three shapes: 1, 32 and 512
candidates of 64 pieces at the initial guess of their scenarios (the first 32 scenarios, repeated), on planning handles with the scenarios' own corridors
(8 faces per cell: 8 lanes per piece, 8 pieces per wave).  The dense check at M = 256 (k_traj_check) is timed beside it on the same handle and data.

Per shape and slack: the _device form timed with HIP events around `--reps` back-to-back launches on one stream after a warm-up launch (the launch
interval).  The initial guesses keep well inside their cells: at slack 0 almost every face is skipped after the quartic task, so the file also records slack
1.0, which pulls the faces through the paths and makes the degree-16 task run.  There is no target: the file records what the kernel does.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="1x64,32x64,512x64", help="candidates x pieces, comma separated")
ap.add_argument("--slacks", default="0,1", help="slacks, comma separated")
ap.add_argument("--kappa", type=int, default=16)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "contain_throughput.json"))
args = ap.parse_args()

import numpy as np  # noqa: E402
import torch  # noqa: E402

from frx_import import frx  # noqa: E402
from fast_racing_amd import scenario as sc  # noqa: E402

torch.cuda.init()                         # torch's HIP runtime first, then the library's (the order bench.py keeps)
if frx.lib().frx_device_count() < 1:
    raise SystemExit("contain_throughput.py needs a HIP device")

stream = torch.cuda.current_stream().cuda_stream


def interval_ms(launch):
    launch()                                                             # warm-up
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.reps):
        launch()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / args.reps


rows = []
for shape in args.shapes.split(","):
    B, N = (int(v) for v in shape.split("x"))
    cands = [sc.make_candidate(b % 32, N, 16) for b in range(B)]
    prob = frx.Problem(cands, sc.ZHANGJIAJIE, qd_intervals=args.kappa)
    T, Cf = prob.forward(prob.initial_guess())
    T = np.ascontiguousarray(T, dtype=np.float64).reshape(-1); Cf = np.ascontiguousarray(Cf, dtype=np.float64).reshape(-1)
    d_T, d_C = torch.from_numpy(T).cuda(), torch.from_numpy(Cf).cuda()
    d_out = torch.zeros(prob.P * 8, dtype=torch.float64, device="cuda")
    check_ms = interval_ms(lambda: prob.trajectory_check_device(d_T.data_ptr(), d_C.data_ptr(), d_out.data_ptr(), 256, stream))
    for slack in (float(v) for v in args.slacks.split(",")):
        ms = interval_ms(lambda: prob.trajectory_contain_device(d_T.data_ptr(), d_C.data_ptr(), d_out.data_ptr(), slack, stream))
        dev = d_out.cpu().numpy().reshape(-1, 8)
        got = prob.trajectory_contain(T, Cf, slack)
        assert np.array_equal(got["piece"], dev, equal_nan=True)
        row = dict(candidates=B, pieces=prob.P, faces_per_piece=prob.Kmax, slack=slack, contain_launch_ms=ms, check_m256_launch_ms=check_ms,
                   ns_per_piece_face=ms * 1e6 / (prob.P * prob.Kmax), contacts=int(got["piece"][:, 0].sum()),
                   pieces_outside=int((got["piece"][:, 1] > 0).sum()), candidates_flagged=int((got["flags"] != 0).sum()))
        rows.append(row)
        print(json.dumps(row), flush=True)
    prob.close()
res = dict(what="frx_trajectory_contain: the _device form's launch interval, k_traj_check at M = 256 beside it", reps=args.reps, rows=rows)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(res, f, indent=1)
