#!/usr/bin/env python3
"""Throughput of the clearance check against the obstacle cloud (frx_trajectory_clearance, csrc/frx_clear_kernel.hpp) at the reference's plan shape
(1 x 64 pieces), the headline batch (32 x 64) and a GPU's Monte-Carlo share (512 x 64), M = 256 intervals, a cloud of 65 536 points, trajectories
at the initial guess.

Per batch: the _device form timed with HIP events around back-to-back launches on one stream (launch interval, us; `--reps` launches, fewer where
one launch takes long), the blocking form timed with a host clock (uploads + launches + download + host reduction), point-sample tests per second,
and a share of the FP64 vector peak.  The kernels' own time comes from a separate run under `rocprofv3 --kernel-trace --stats` (pass --reps small
there); `--merge-trace` adds it to an existing result file by the grid size of each batch's launches; DESIGN.md 3.11 quotes both.

Operation count (nominal, from the kernel's expressions, per point-sample test; compares, min / max and selects count 0):
  u = o - p                                      3 add
  three axis.u products                          3 mul + 6 fma
  q = d0^2 + d1^2 + d2^2                         1 mul + 2 fma
  r = u.u                                        1 mul + 2 fma
so 18 FP64 instructions = 28 flops (an FMA counts 2) per test; the sample states (once per sample and pass of 1024 points) are left out.
Peak: 78.6 TFLOP/s, the MI355X datasheet's FP64 vector figure.
"""
import argparse
import csv
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FLOP_TEST, INSTR_TEST = 28, 18
FP64_VECTOR_PEAK = 78.6e12

ap = argparse.ArgumentParser()
ap.add_argument("--intervals", type=int, default=256)
ap.add_argument("--points", type=int, default=65536)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--batches", default="1,32,512")
ap.add_argument("--out", default="", help="write the JSON result here as well")
ap.add_argument("--merge-trace", default="", help="a rocprofv3 kernel-trace CSV: add the kernels' own time per batch to the file given by --out and leave")
args = ap.parse_args()

if args.merge_trace:
    with open(args.out) as f:
        res = json.load(f)
    by_grid = {}
    with open(args.merge_trace) as f:
        for rec in csv.DictReader(f):
            if "k_traj_clear" in rec["Kernel_Name"]:
                key = ("reduce" if "reduce" in rec["Kernel_Name"] else "main", int(rec["Grid_Size_X"]) // int(rec["Workgroup_Size_X"]))
                by_grid.setdefault(key, []).append((int(rec["End_Timestamp"]) - int(rec["Start_Timestamp"])) * 1e-3)
    for row in res["rows"]:
        main = by_grid.get(("main", row["pieces"] * row["chunks"]), [])
        red = by_grid.get(("reduce", (row["pieces"] + 3) // 4), []) if row["chunks"] > 1 else []
        if main:
            row["kernel_us_rocprofv3"] = dict(k_traj_clear=sorted(main)[len(main) // 2], k_traj_clear_reduce=sorted(red)[len(red) // 2] if red else 0.0,
                                              dispatches=len(main))
            us = row["kernel_us_rocprofv3"]["k_traj_clear"] + row["kernel_us_rocprofv3"]["k_traj_clear_reduce"]
            row["kernel_tests_per_s"] = row["tests"] / (us * 1e-6)
            row["kernel_fp64_vector_peak_share"] = row["flops"] / (us * 1e-6) / FP64_VECTOR_PEAK
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    raise SystemExit(0)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from frx_import import frx  # noqa: E402
from fast_racing_amd import scenario as sc  # noqa: E402

torch.cuda.init()                         # torch's HIP runtime first, then the library's (the order bench.py keeps)
if frx.lib().frx_device_count() < 1:
    raise SystemExit("clear_throughput.py needs a HIP device")

_, N, gates, kappa = sc.CONFIGS["headline"]
M, n_obs = args.intervals, args.points
rows = []
stream = torch.cuda.current_stream().cuda_stream
for B in [int(b) for b in args.batches.split(",")]:
    # 1: the reference's only plan shape; 32: the headline batch (gate perturbations of one scenario); 512: a GPU's share of the Monte-Carlo config
    cands = sc.make_batch(0, B, N, gates) if B <= 32 else [sc.make_candidate(b, N, gates) for b in range(B)]
    prob = frx.Problem(cands, sc.ZHANGJIAJIE, qd_intervals=kappa)
    T, Cf = prob.forward(prob.initial_guess())
    # a cloud over the bounding box of the batch's own positions, one metre around it: near enough that no test is trivially far
    p0 = np.asarray(Cf).reshape(-1, 6, 3)[:, 0]
    obs = np.random.default_rng(B).uniform(p0.min(axis=0) - 1.0, p0.max(axis=0) + 1.0, (n_obs, 3))
    tests = float(prob.P) * (M + 1) * n_obs
    flops = tests * FLOP_TEST
    nbytes = prob.trajectory_clearance_workspace(n_obs, M)
    chunks = max(1, nbytes // (32 * prob.P))
    Td = torch.from_numpy(T).cuda(); Cd = torch.from_numpy(np.ascontiguousarray(Cf).reshape(-1)).cuda(); Od = torch.from_numpy(obs.reshape(-1)).cuda()
    Wd = torch.zeros(max(nbytes // 8, 1), dtype=torch.float64, device="cuda")
    out = torch.zeros(prob.P * 4, dtype=torch.float64, device="cuda")

    def launch():
        prob.trajectory_clearance_device(Td.data_ptr(), Cd.data_ptr(), Od.data_ptr(), n_obs, Wd.data_ptr() if nbytes else 0, out.data_ptr(), M, stream)
    reps = int(max(2, min(args.reps, 4e12 / tests)))                      # (a launch of the largest batch runs for a third of a second)
    launch()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        launch()
    e1.record()
    torch.cuda.synchronize()
    us_dev = e0.elapsed_time(e1) * 1e3 / reps
    r = prob.trajectory_clearance(T, Cf, obs, M)
    t0 = time.perf_counter()
    for _ in range(2):
        r = prob.trajectory_clearance(T, Cf, obs, M)
    us_blk = (time.perf_counter() - t0) * 1e6 / 2
    assert np.array_equal(out.cpu().numpy().reshape(-1, 4), r["piece"])
    rows.append(dict(batch=B, pieces=prob.P, intervals=M, points=n_obs, chunks=int(chunks), workgroups=int(prob.P * chunks), tests=tests, flops=flops, reps=reps,
                     device_launch_us=us_dev, blocking_call_us=us_blk, tests_per_s=tests / (us_dev * 1e-6),
                     gflops=flops / (us_dev * 1e-6) / 1e9, fp64_vector_peak_share=flops / (us_dev * 1e-6) / FP64_VECTOR_PEAK,
                     min_ell=float(r["ell"].min()), collisions=int((r["flags"] & frx.CLEAR_FLAG_COLLISION != 0).sum())))
    print(json.dumps(rows[-1]), flush=True)
    prob.close()
res = dict(what="frx_trajectory_clearance throughput", flop_model=dict(flops_per_test=FLOP_TEST, fp64_instructions_per_test=INSTR_TEST,
                                                                         peak_flops=FP64_VECTOR_PEAK), rows=rows)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
