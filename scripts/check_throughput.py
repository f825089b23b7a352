#!/usr/bin/env python3
"""Throughput of the dense feasibility check (frx_trajectory_check, csrc/frx_check_kernel.hpp) at the headline batch (32 x 64 pieces) and a GPU's
Monte-Carlo share (512 x 64), M = 256 check intervals, trajectories at the initial guess.

Per batch: the _device form timed with HIP events around `--reps` back-to-back launches on one stream (launch interval, us), the blocking form timed
with a host clock (uploads + launch + download + host reduction, us), samples per second, and a share of the FP64 vector peak.  The kernel's own
time comes from a separate run under `rocprofv3 --kernel-trace --stats` (pass --reps small there); DESIGN.md §3.9 quotes both.

FLOP count (nominal, from the kernel's expressions; an FMA counts 2, a square root or reciprocal square root 1, compares 0):
  per sample   quintic position / velocity / acceleration / jerk at s (powers of s shared by the three axes)        103
               frame (h, |h|^2, rsqrt, zB, yB, xB)                                                                    45
               limits (|v|, |a|, |h|, R^T j and |omega_xy|)                                                            27
               origin shift of the position                                                                            3
  per sample and half-space: R^T n scaled by the ellipsoid, its norm, n.(p - org), margin, sum                       30
so a piece with K half-spaces costs (M + 1)(178 + 30 K) flops.  Peak: 78.6 TFLOP/s, the MI355X datasheet's FP64 vector figure.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from frx_import import frx  # noqa: E402
from fast_racing_amd import scenario as sc  # noqa: E402

FLOP_SAMPLE, FLOP_HALFSPACE = 178, 30
FP64_VECTOR_PEAK = 78.6e12

ap = argparse.ArgumentParser()
ap.add_argument("--intervals", type=int, default=256)
ap.add_argument("--reps", type=int, default=200)
ap.add_argument("--batches", default="32,512")
ap.add_argument("--out", default="", help="write the JSON result here as well")
args = ap.parse_args()
torch.cuda.init()                         # torch's HIP runtime first, then the library's (the order bench.py keeps)
if frx.lib().frx_device_count() < 1:
    raise SystemExit("check_throughput.py needs a HIP device")

_, N, gates, kappa = sc.CONFIGS["headline"]
M = args.intervals
rows = []
stream = torch.cuda.current_stream().cuda_stream
for B in [int(b) for b in args.batches.split(",")]:
    # 32: the headline batch (gate perturbations of one scenario); 512: a GPU's share of the Monte-Carlo config (independent scenarios)
    cands = sc.make_batch(0, B, N, gates) if B <= 32 else [sc.make_candidate(b, N, gates) for b in range(B)]
    prob = frx.Problem(cands, sc.ZHANGJIAJIE, qd_intervals=kappa)
    T, Cf = prob.forward(prob.initial_guess())
    K = np.array([h.shape[1] for c in cands for h in c.h_polys])
    flops = float((M + 1) * (FLOP_SAMPLE * len(K) + FLOP_HALFSPACE * K.sum()))
    samples = prob.P * (M + 1)
    Td = torch.from_numpy(T).cuda(); Cd = torch.from_numpy(np.ascontiguousarray(Cf).reshape(-1)).cuda()
    out = torch.zeros(prob.P * 8, dtype=torch.float64, device="cuda")
    for _ in range(10):
        prob.trajectory_check_device(Td.data_ptr(), Cd.data_ptr(), out.data_ptr(), M, stream)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.reps):
        prob.trajectory_check_device(Td.data_ptr(), Cd.data_ptr(), out.data_ptr(), M, stream)
    e1.record()
    torch.cuda.synchronize()
    us_dev = e0.elapsed_time(e1) * 1e3 / args.reps
    for _ in range(5):
        prob.trajectory_check(T, Cf, M)
    t0 = time.perf_counter()
    for _ in range(args.reps):
        r = prob.trajectory_check(T, Cf, M)
    us_blk = (time.perf_counter() - t0) * 1e6 / args.reps
    assert np.array_equal(out.cpu().numpy().reshape(-1, 8), r["piece"])
    rows.append(dict(batch=B, pieces=prob.P, intervals=M, half_spaces=int(K.sum()), samples=samples, flops=flops,
                     device_launch_us=us_dev, blocking_call_us=us_blk, samples_per_s=samples / (us_dev * 1e-6),
                     gflops=flops / (us_dev * 1e-6) / 1e9, fp64_vector_peak_share=flops / (us_dev * 1e-6) / FP64_VECTOR_PEAK,
                     flagged=int((r["flags"] != 0).sum())))
    print(json.dumps(rows[-1]), flush=True)
    prob.close()
res = dict(what="frx_trajectory_check throughput", flop_model=dict(per_sample=FLOP_SAMPLE, per_sample_and_half_space=FLOP_HALFSPACE,
                                                                   peak_flops=FP64_VECTOR_PEAK), rows=rows)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
