#!/usr/bin/env python3
"""Throughput of batched trajectory sampling (frx_trajectory_sample, csrc/frx_sample_kernel.hpp), trajectories at the initial guess:
  headline   the headline batch (32 x 64 pieces) at 1 kHz over each trajectory (dt = 1 ms, S = the longest duration / dt + 1)
  mc512      a GPU's Monte-Carlo share (512 x 64 pieces) at S = 8192 samples spread over each duration: 4.2 M rows, 671 MB written

Per case: the _device form timed with HIP events around `--reps` back-to-back launches on one stream (launch interval, us), the blocking form
timed with a host clock (upload of T and C, launch, download of every row into host memory, us), and the bytes the kernel writes (160 per row)
per second against the store rate MI355X_MICROARCH.md measures for plain stores, 6.0-6.2 TB/s.  The kernel's own time comes from a separate run
under `rocprofv3 --kernel-trace --stats`; `--merge-trace` folds that run's kernel trace CSV into the JSON (medians per grid size, in the order
the cases ran).  DESIGN.md §3.10 quotes the numbers.
"""
import argparse
import csv
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

STORE_RATE = 6.1e12                       # bytes/s, plain stores (MI355X_MICROARCH.md, "Global float atomics": 6.0-6.2 TB/s)
ROW_BYTES = 160

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=200)
ap.add_argument("--blocking-reps", type=int, default=10)
ap.add_argument("--cases", default="headline,mc512")
ap.add_argument("--out", default="", help="write the JSON result here as well")
ap.add_argument("--merge-trace", default="", help="rocprofv3 kernel trace CSV of a run of this script: add its k_traj_sample times to --out")
args = ap.parse_args()

if args.merge_trace:
    with open(args.out) as f:
        res = json.load(f)
    groups = {}
    with open(args.merge_trace) as f:
        for r in csv.DictReader(f):
            if "k_traj_sample" in r["Kernel_Name"]:
                groups.setdefault(int(r["Grid_Size_X"]), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3)
    for row, (grid, us) in zip(res["rows"], groups.items()):    # (dicts keep the order of first appearance: the order the cases ran)
        us = np.array(us)
        row["kernel_us_rocprofv3"] = dict(median=float(np.median(us)), min=float(us.min()), max=float(us.max()), launches=len(us), workgroups=grid // 256)
        k = row["kernel_us_rocprofv3"]["median"] * 1e-6
        row["kernel_bytes_per_s"] = row["bytes_written"] / k
        row["kernel_store_rate_share"] = row["bytes_written"] / k / STORE_RATE
    res["source"] += f"; kernel_us_rocprofv3 from a separate run under rocprofv3 --kernel-trace --stats ({os.path.basename(args.merge_trace)})"
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res["rows"], indent=1))
    sys.exit(0)

import torch  # noqa: E402

torch.cuda.init()                         # torch's HIP runtime first, then the library's (the order bench.py keeps)
from frx_import import frx  # noqa: E402
from fast_racing_amd import scenario as sc  # noqa: E402

if frx.lib().frx_device_count() < 1:
    raise SystemExit("sample_throughput.py needs a HIP device")

_, N, gates, kappa = sc.CONFIGS["headline"]
rows = []
stream = torch.cuda.current_stream().cuda_stream
for case in args.cases.split(","):
    B = 32 if case == "headline" else 512
    # 32: gate perturbations of one scenario; 512: independent scenarios
    cands = sc.make_batch(0, B, N, gates) if case == "headline" else [sc.make_candidate(b, N, gates) for b in range(B)]
    prob = frx.Problem(cands, sc.ZHANGJIAJIE, qd_intervals=kappa)
    T, Cf = prob.forward(prob.initial_guess())
    totals = np.add.reduceat(T, prob.piece_off[:-1])
    if case == "headline":
        dt = 1e-3
        S = int(np.floor(totals.max() / dt)) + 1
    else:
        dt, S = 0.0, 8192
    nbytes = B * S * ROW_BYTES
    Td = torch.from_numpy(T).cuda(); Cd = torch.from_numpy(np.ascontiguousarray(Cf).reshape(-1)).cuda()
    out = torch.empty(B * S * 20, dtype=torch.float64, device="cuda")
    for _ in range(10):
        prob.trajectory_sample_device(Td.data_ptr(), Cd.data_ptr(), out.data_ptr(), S, dt=dt, stream=stream)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.reps):
        prob.trajectory_sample_device(Td.data_ptr(), Cd.data_ptr(), out.data_ptr(), S, dt=dt, stream=stream)
    e1.record()
    torch.cuda.synchronize()
    us_dev = e0.elapsed_time(e1) * 1e3 / args.reps
    for _ in range(2):
        r = prob.trajectory_sample(T, Cf, S, dt=dt)
    t0 = time.perf_counter()
    for _ in range(args.blocking_reps):
        r = prob.trajectory_sample(T, Cf, S, dt=dt)
    us_blk = (time.perf_counter() - t0) * 1e6 / args.blocking_reps
    assert np.array_equal(out.cpu().numpy().reshape(B, S, 20), r["rows"])
    rows.append(dict(case=case, batch=B, pieces=prob.P, n_samples=S, dt=dt, rows=B * S, bytes_written=nbytes, longest_duration_s=float(totals.max()),
                     device_launch_us=us_dev, blocking_call_us=us_blk, bytes_per_s=nbytes / (us_dev * 1e-6),
                     store_rate_share=nbytes / (us_dev * 1e-6) / STORE_RATE, max_thrust=float(r["thrust"].max()), max_body_rate_xy=float(np.linalg.norm(r["omega"][..., :2], axis=2).max())))
    print(json.dumps(rows[-1]), flush=True)
    del out, r
    prob.close()
res = dict(what="frx_trajectory_sample throughput", store_rate=STORE_RATE, row_bytes=ROW_BYTES,
           source="scripts/sample_throughput.py (HIP events, host clock)", rows=rows)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
