#!/usr/bin/env python3
"""Throughput of the exact clearance certificate (frx_trajectory_clearance_exact, csrc/frx_clear_exact_kernel.hpp) at the reference's plan shape (1 x 64
pieces), the headline batch (32 x 64) and 256 x 64, a cloud of 65 536 points, trajectories at the initial guess.  The entry has no M: nothing is sampled.

Per batch: the _device form timed with HIP events around back-to-back launches on one stream (launch interval, us: the bounds kernel, the certificate
kernel and the fold of the chunks together), the blocking form timed with a host clock (uploads + launches + download + host fold), and what the cull left:
survivors and degree-21 tasks per piece (frx_debug_clear_exact_counts).  For scale, the dense form's launch interval at M = 256 on the same inputs.
The cloud is spread over the bounding box of the batch's own positions, one metre round it, as scripts/clear_throughput.py spreads it: ONE synthetic
scenario - how many survivors a real cloud leaves nobody has measured.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ap = argparse.ArgumentParser()
ap.add_argument("--points", type=int, default=65536)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--batches", default="1,32,256")
ap.add_argument("--dense-intervals", type=int, default=256)
ap.add_argument("--out", default="", help="write the JSON result here as well")
args = ap.parse_args()

import numpy as np  # noqa: E402
import torch  # noqa: E402

from frx_import import frx  # noqa: E402
from fast_racing_amd import scenario as sc  # noqa: E402

torch.cuda.init()                         # torch's HIP runtime first, then the library's (the order bench.py keeps)
if frx.lib().frx_device_count() < 1:
    raise SystemExit("clear_exact_throughput.py needs a HIP device")

_, N, gates, kappa = sc.CONFIGS["headline"]
n_obs, M = args.points, args.dense_intervals
rows = []
stream = torch.cuda.current_stream().cuda_stream


def interval_us(launch, reps):
    launch()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        launch()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


for B in [int(b) for b in args.batches.split(",")]:
    cands = sc.make_batch(0, B, N, gates) if B <= 32 else [sc.make_candidate(b, N, gates) for b in range(B)]
    prob = frx.Problem(cands, sc.ZHANGJIAJIE, qd_intervals=kappa)
    T, Cf = prob.forward(prob.initial_guess())
    p0 = np.asarray(Cf).reshape(-1, 6, 3)[:, 0]
    obs = np.random.default_rng(B).uniform(p0.min(axis=0) - 1.0, p0.max(axis=0) + 1.0, (n_obs, 3))
    nbytes = prob.trajectory_clearance_exact_workspace(n_obs)
    chunks = nbytes // (80 * prob.P)
    Td = torch.from_numpy(T).cuda(); Cd = torch.from_numpy(np.ascontiguousarray(Cf).reshape(-1)).cuda(); Od = torch.from_numpy(obs.reshape(-1)).cuda()
    Wd = torch.zeros(nbytes // 8, dtype=torch.float64, device="cuda")
    out = torch.zeros(prob.P * 6, dtype=torch.float64, device="cuda")

    def launch():
        prob.trajectory_clearance_exact_device(Td.data_ptr(), Cd.data_ptr(), Od.data_ptr(), n_obs, Wd.data_ptr(), out.data_ptr(), stream)
    us_dev = interval_us(launch, args.reps)
    surv, ell = prob.clear_exact_counts()
    r = prob.trajectory_clearance_exact(T, Cf, obs)
    t0 = time.perf_counter()
    for _ in range(2):
        r = prob.trajectory_clearance_exact(T, Cf, obs)
    us_blk = (time.perf_counter() - t0) * 1e6 / 2
    assert np.array_equal(out.cpu().numpy().reshape(-1, 6), r["piece"], equal_nan=True)
    # the dense form on the same inputs
    dbytes = prob.trajectory_clearance_workspace(n_obs, M)
    Wdd = torch.zeros(max(dbytes // 8, 1), dtype=torch.float64, device="cuda")
    dout = torch.zeros(prob.P * 4, dtype=torch.float64, device="cuda")

    def dense():
        prob.trajectory_clearance_device(Td.data_ptr(), Cd.data_ptr(), Od.data_ptr(), n_obs, Wdd.data_ptr() if dbytes else 0, dout.data_ptr(), M, stream)
    us_dense = interval_us(dense, max(2, min(args.reps, int(4e12 / (float(prob.P) * (M + 1) * n_obs)))))
    d = dout.cpu().numpy().reshape(-1, 4)
    rows.append(dict(batch=B, pieces=prob.P, points=n_obs, chunks=int(chunks), workgroups=int(prob.P * chunks), reps=args.reps,
                     device_launch_us=us_dev, blocking_call_us=us_blk, us_per_piece=us_dev / prob.P,
                     survivors_per_piece=dict(mean=float(surv.mean()), max=int(surv.max())), ell_tasks_per_piece=dict(mean=float(ell.mean()), max=int(ell.max())),
                     dense_intervals=M, dense_launch_us=us_dense, min_ell=float(r["ell"].min()), dense_min_ell=float(d[:, 0].min()),
                     largest_dense_minus_exact_ell=float((d[:, 0] - r["piece"][:, 0]).max()),
                     collisions=int((r["flags"] & frx.CLEAR_FLAG_COLLISION != 0).sum())))
    print(json.dumps(rows[-1]), flush=True)
    prob.close()
res = dict(what="frx_trajectory_clearance_exact throughput (one synthetic scenario: a cloud spread over the batch's bounding box)", rows=rows)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
