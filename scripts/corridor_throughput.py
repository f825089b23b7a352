#!/usr/bin/env python3
"""Throughput of whole-corridor generation on the device (frx_corridor_generate_batch, csrc/frx_chain_kernel.hpp): 1, 32 and 512 routes of about 64 cells each
(20 gates, about 270 m at 0.5 m spacing) through ONE cloud of 4 096 and of 65 536 points and the voxel map marked from it, against the host chain
frx_corridor_generate on the same machine and the same routes, one host thread, sight lines by frx_map_is_blocked.

Per (routes, points): the _device form timed with HIP events around `--reps` back-to-back launches on one stream, the blocking form with a host clock (uploads,
launch, download, compaction), the host chain with a host clock over the first `--host-routes` routes (per-route time; the batch's host time is that times the
routes, marked as extrapolated when not all were run).  The kernel's own time comes from a separate run under `rocprofv3 --kernel-trace --stats` with
`--kernel-only` (one launch per configuration, in the order of the rows); `--merge-trace` adds it to the file given by --out.  DESIGN.md 3.12 quotes the table.
"""
import argparse
import csv
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ap = argparse.ArgumentParser()
ap.add_argument("--routes", default="1,32,512")
ap.add_argument("--points", default="4096,65536")
ap.add_argument("--gates", type=int, default=20)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--host-routes", type=int, default=8, help="routes the host chain is timed on per configuration (0: skip the baseline)")
ap.add_argument("--kernel-only", action="store_true", help="one device-form launch per configuration and nothing else (for a rocprofv3 run)")
ap.add_argument("--out", default="")
ap.add_argument("--merge-trace", default="", help="a rocprofv3 kernel-trace CSV of a --kernel-only run: add the kernel's time per row to the file given by --out and leave")
args = ap.parse_args()

if args.merge_trace:
    with open(args.out) as f:
        res = json.load(f)
    with open(args.merge_trace) as f:
        disp = sorted((int(r["Start_Timestamp"]), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3, int(r["Grid_Size_X"]) // int(r["Workgroup_Size_X"]))
                      for r in csv.DictReader(f) if "k_corridor_chain" in r["Kernel_Name"])
    assert len(disp) == len(res["rows"]), (len(disp), len(res["rows"]))
    for row, (_, us, grid) in zip(res["rows"], disp):
        assert grid == row["routes"], (grid, row["routes"])
        row["kernel_us_rocprofv3"] = us
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    raise SystemExit(0)

import ctypes as C  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

from frx_import import frx  # noqa: E402
from fast_racing_amd import scenario as sc  # noqa: E402

torch.cuda.init()                         # torch's HIP runtime first, then the library's (the order bench.py keeps)
if frx.lib().frx_device_count() < 1:
    raise SystemExit("corridor_throughput.py needs a HIP device")

BBOX, HEIGHT, MAX_SEG, RES = np.array(sc.ZHANGJIAJIE["polyhedron_box"], dtype=float), sc.ZHANGJIAJIE["map_height"], 4.0, 0.25
CAP_POLYS, CAP_PLANES = 128, 64


def route(seed):
    gates = sc.make_gates(sc.SplitMix64(seed), args.gates)
    wps = np.vstack([[0.0, 0.0, 1.0], gates, gates[-1] + [0.0, 14.8, 0.0]])
    path = [wps[0]]
    for a, b in zip(wps[:-1], wps[1:]):
        m = int(np.ceil(np.linalg.norm(b - a) / 0.5))
        path += [a + (b - a) * (t / m) for t in range(1, m + 1)]
    return np.array(path)


def cloud(rng, paths, n, lo, hi):
    """n uniform points in the routes' bounding volume, none within 0.5 m (one cell of a 0.5 m grid, and its neighbours) of a route point"""
    pts = np.vstack(paths)
    dim = np.ceil((hi - lo) / 0.5).astype(int) + 1
    near = np.zeros(dim, bool)
    c = ((pts - lo) / 0.5).astype(int)
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dz in (-1, 0, 1):
                q = np.clip(c + [dx, dy, dz], 0, dim - 1)
                near[q[:, 0], q[:, 1], q[:, 2]] = True
    out = np.zeros((0, 3))
    while len(out) < n:
        q = rng.uniform(lo, hi, (2 * n, 3))
        k = ((q - lo) / 0.5).astype(int)
        out = np.vstack([out, q[~near[k[:, 0], k[:, 1], k[:, 2]]]])
    return out[:n]


rows = []
stream = torch.cuda.current_stream().cuda_stream
all_routes = [route(1000 + b) for b in range(max(int(b) for b in args.routes.split(",")))]
for n_obs in [int(p) for p in args.points.split(",")]:
    for B in [int(b) for b in args.routes.split(",")]:
        paths = all_routes[:B]
        pts = np.vstack(all_routes)                                         # one world for every batch size: the cloud does not depend on B
        lo = np.array([pts[:, 0].min() - 6.0, pts[:, 1].min() - 6.0, 0.0]); hi = np.array([pts[:, 0].max() + 6.0, pts[:, 1].max() + 6.0, HEIGHT])
        obs = cloud(np.random.default_rng(n_obs), all_routes, n_obs, lo, hi)
        vm = frx.VoxelMap(lo - [0.0, 0.0, 0.5], np.ceil((hi - lo + [0.0, 0.0, 1.0]) / RES).astype(int), RES)
        vm.mark_cloud(obs)
        off = np.zeros(B + 1, np.int32); off[1:] = np.cumsum([len(p) for p in paths])
        d_off = torch.from_numpy(off).cuda(); d_path = torch.from_numpy(np.concatenate(paths).reshape(-1)).cuda(); d_obs = torch.from_numpy(obs.reshape(-1)).cuda()
        d_cells = torch.from_numpy(vm.cells).cuda()
        d_slot = torch.zeros(B * CAP_POLYS * CAP_PLANES * 6, dtype=torch.float64, device="cuda"); d_cp = torch.zeros(B * CAP_POLYS, dtype=torch.int32, device="cuda")
        d_np = torch.zeros(B, dtype=torch.int32, device="cuda"); d_st = torch.zeros(B, dtype=torch.int32, device="cuda")
        ms = frx.VoxelMapStruct((C.c_double * 3)(*vm.origin), (C.c_int * 3)(*[int(d) for d in vm.dim]), vm.res, d_cells.data_ptr())

        def launch():
            frx.corridor_generate_batch_device(B, d_off.data_ptr(), d_path.data_ptr(), n_obs, d_obs.data_ptr(), BBOX, HEIGHT, MAX_SEG, ms, CAP_POLYS, CAP_PLANES,
                                               d_slot.data_ptr(), d_cp.data_ptr(), d_np.data_ptr(), d_st.data_ptr(), stream)
        launch()
        torch.cuda.synchronize()
        n_polys, status = d_np.cpu().numpy(), d_st.cpu().numpy()
        row = dict(routes=B, points=n_obs, path_points=int(off[-1]), cells=int(n_polys.sum()), cells_per_route=float(n_polys.mean()), failed_routes=int((status != 0).sum()))
        if not args.kernel_only:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.reps):
                launch()
            e1.record()
            torch.cuda.synchronize()
            row["device_launch_ms"] = e0.elapsed_time(e1) / args.reps
            frx.corridor_generate_batch(paths, obs, BBOX, HEIGHT, MAX_SEG, blocked=vm, cap_polys=CAP_POLYS, cap_planes=CAP_PLANES, raw=True)
            t0 = time.perf_counter()
            blk = frx.corridor_generate_batch(paths, obs, BBOX, HEIGHT, MAX_SEG, blocked=vm, cap_polys=CAP_POLYS, cap_planes=CAP_PLANES, raw=True)
            row["blocking_call_ms"] = (time.perf_counter() - t0) * 1e3
            assert np.array_equal(blk[0], n_polys)
            nh = min(B, args.host_routes)
            if nh:
                t0 = time.perf_counter()
                host = [frx.corridor_generate(p, obs, BBOX, HEIGHT, MAX_SEG, blocked=vm) for p in paths[:nh]]
                ms_route = (time.perf_counter() - t0) * 1e3 / nh
                row["host_routes_with_equal_cell_count"] = int(sum(len(h) == int(v) for h, v in zip(host, n_polys[:nh])))   # (these worlds are not made decision-safe)
                row.update(host_ms_per_route=ms_route, host_routes_measured=nh, host_ms_batch=ms_route * B, host_ms_batch_extrapolated=bool(nh < B),
                           speedup_device_launch=ms_route * B / row["device_launch_ms"], speedup_blocking_call=ms_route * B / row["blocking_call_ms"])
        rows.append(row)
        print(json.dumps(row), flush=True)
res = dict(what="frx_corridor_generate_batch throughput against the host chain", cap_polys=CAP_POLYS, cap_planes=CAP_PLANES, gates=args.gates, rows=rows)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
