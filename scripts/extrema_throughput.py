#!/usr/bin/env python3
"""Throughput of the exact per-piece extrema on the device (frx_trajectory_extrema, csrc/frx_extrema_kernel.hpp): batches of 1, 32 and 512 candidates of 64
pieces at the initial guess, against the host's frx_traj_max_rates on one thread of the same machine (two of the five quantities) and against the sampling
check k_traj_check at M = 256 on the same batch.

Per batch: the _device form timed with HIP events around `--reps` back-to-back launches on one stream after a warm-up launch (the launch interval), the
blocking form with a host clock (upload, launch, download, reduction), frx_traj_max_rates with a host clock, frx_trajectory_check_device with events.
The kernel's own time comes from a separate run under `rocprofv3 --kernel-trace --stats` with `--kernel-only` (a warm-up and one timed launch per batch, in the
order of the rows); `--merge-trace` adds it to the file given by --out.  DESIGN.md 3.16 quotes the table.
"""
import argparse
import csv
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--batches", default="1,32,512")
ap.add_argument("--pieces", type=int, default=64)
ap.add_argument("--gates", type=int, default=16)
ap.add_argument("--kappa", type=int, default=16)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--check-intervals", type=int, default=256)
ap.add_argument("--kernel-only", action="store_true", help="a warm-up and one device-form launch per batch and nothing else (for a rocprofv3 run)")
ap.add_argument("--out", default="")
ap.add_argument("--merge-trace", default="", help="a rocprofv3 kernel-trace CSV of a --kernel-only run: add the kernel's time per row to the file given by --out and leave")
args = ap.parse_args()

if args.merge_trace:
    with open(args.out) as f:
        res = json.load(f)
    with open(args.merge_trace) as f:
        disp = sorted((int(r["Start_Timestamp"]), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3, int(r["Grid_Size_X"]) // int(r["Workgroup_Size_X"]))
                      for r in csv.DictReader(f) if "k_traj_extrema" in r["Kernel_Name"])
    assert len(disp) == 2 * len(res["rows"]), (len(disp), len(res["rows"]))
    for row, (_, us, grid) in zip(res["rows"], disp[1::2]):               # the second launch of every pair: after the warm-up
        assert grid == (row["pieces"] + 63) // 64, (grid, row["pieces"])
        row["kernel_us_rocprofv3"] = us
        row["kernel_ns_per_piece"] = us * 1e3 / row["pieces"]
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    raise SystemExit(0)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from frx_import import frx  # noqa: E402
from fast_racing_amd import scenario as sc  # noqa: E402

torch.cuda.init()                         # torch's HIP runtime first, then the library's (the order bench.py keeps)
if frx.lib().frx_device_count() < 1:
    raise SystemExit("extrema_throughput.py needs a HIP device")

stream = torch.cuda.current_stream().cuda_stream
made = {}
rows = []
for B in [int(b) for b in args.batches.split(",")]:
    cands = []
    for b in range(B):                                                   # 32 different scenarios, repeated: a launch's time depends on the pieces, not on their corridors
        if b % 32 not in made:
            made[b % 32] = sc.make_candidate(b % 32, args.pieces, args.gates)
        cands.append(made[b % 32])
    prob = frx.Problem(cands, sc.ZHANGJIAJIE, qd_intervals=args.kappa)
    T, Cf = prob.forward(prob.initial_guess())
    T = np.ascontiguousarray(T); Cf = np.ascontiguousarray(Cf).reshape(-1)
    d_T = torch.from_numpy(T).cuda(); d_C = torch.from_numpy(Cf).cuda()
    d_out = torch.zeros(prob.P * 10, dtype=torch.float64, device="cuda"); d_chk = torch.zeros(prob.P * 8, dtype=torch.float64, device="cuda")

    def launch():
        prob.trajectory_extrema_device(d_T.data_ptr(), d_C.data_ptr(), d_out.data_ptr(), stream)

    def launch_check():
        prob.trajectory_check_device(d_T.data_ptr(), d_C.data_ptr(), d_chk.data_ptr(), args.check_intervals, stream)

    def timed(fn):
        fn()                                                             # warm-up
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.reps
    row = dict(candidates=B, pieces=int(prob.P))
    if args.kernel_only:
        launch(); launch()
        torch.cuda.synchronize()
    else:
        row["device_launch_ms"] = timed(launch)
        rows_dev = d_out.cpu().numpy().reshape(-1, 10)
        prob.trajectory_extrema(T, Cf)
        t0 = time.perf_counter()
        got = prob.trajectory_extrema(T, Cf)
        row["blocking_call_ms"] = (time.perf_counter() - t0) * 1e3
        assert np.array_equal(got["piece"], rows_dev, equal_nan=True)
        frx.traj_max_rates(T[:64], Cf[:64 * 18].reshape(-1, 3))
        t0 = time.perf_counter()
        mv, ma = frx.traj_max_rates(T, Cf.reshape(-1, 3))
        row["host_max_rates_ms_1_thread"] = (time.perf_counter() - t0) * 1e3
        row["host_max_rates_us_per_piece"] = row["host_max_rates_ms_1_thread"] * 1e3 / prob.P
        row["host_rows_equal_bit_for_bit"] = int((np.equal(mv, got["piece"][:, 0]) & np.equal(ma, got["piece"][:, 1])).sum())   # (all but the host's early-outs)
        row["check_m%d_launch_ms" % args.check_intervals] = timed(launch_check)
        row["nonfinite_rows"] = int((~np.isfinite(got["piece"])).any(axis=1).sum())
    rows.append(row)
    print(json.dumps(row), flush=True)
    prob.close()
res = dict(what="frx_trajectory_extrema throughput against frx_traj_max_rates on the host and k_traj_check on the device", pieces_per_candidate=args.pieces,
           check_intervals=args.check_intervals, reps=args.reps, rows=rows)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
