#!/usr/bin/env python3
"""Throughput of the H -> V vertex enumeration on the device (frx_enumerate_vertices_batch, csrc/frx_enumerate_kernel.hpp): the cells and overlaps of 1, 32 and
512 routes' corridors in clouds of 3 000 and of 20 000 points, against the host's frx_enumerate_vertices on the same machine and the same polytopes.

The corridors are generated ONCE on the host (frx_corridor_generate) for `--base-routes` routes of tests/corridor_states.py's kind through one cloud; a batch of
B routes replicates them in turn, each replica shifted by a translation of its own (same shapes, other numbers).  Per (routes, points): the _device form timed
with HIP events around `--reps` back-to-back launches on one stream, the blocking form with a host clock (task list, uploads, launch, download, compaction), and
frx_enumerate_vertices called polytope by polytope on one host thread and on `--threads` threads of this process (the call releases the interpreter lock),
over the first `--host-polys` polytopes (per-polytope time; the batch's host time is that times the polytopes, marked as extrapolated when not all were run).
The kernel's own time comes from a separate run under `rocprofv3 --kernel-trace --stats` with `--kernel-only` (one launch per configuration, in the order of the
rows); `--merge-trace` adds it to the file given by --out.  DESIGN.md 3.15 quotes the table.
"""
import argparse
import csv
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

ap = argparse.ArgumentParser()
ap.add_argument("--routes", default="1,32,512")
ap.add_argument("--points", default="3000,20000")
ap.add_argument("--base-routes", type=int, default=7)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--cap-v", type=int, default=96)
ap.add_argument("--threads", type=int, default=16)
ap.add_argument("--host-polys", type=int, default=2000, help="polytopes the host function is timed on per configuration (0: skip the baseline)")
ap.add_argument("--kernel-only", action="store_true", help="one device-form launch per configuration and nothing else (for a rocprofv3 run)")
ap.add_argument("--out", default="")
ap.add_argument("--merge-trace", default="", help="a rocprofv3 kernel-trace CSV of a --kernel-only run: add the kernel's time per row to the file given by --out and leave")
args = ap.parse_args()

if args.merge_trace:
    with open(args.out) as f:
        res = json.load(f)
    with open(args.merge_trace) as f:
        disp = sorted((int(r["Start_Timestamp"]), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3, int(r["Grid_Size_X"]) // int(r["Workgroup_Size_X"]))
                      for r in csv.DictReader(f) if "k_enumerate" in r["Kernel_Name"])
    assert len(disp) == len(res["rows"]), (len(disp), len(res["rows"]))
    for row, (_, us, grid) in zip(res["rows"], disp):
        assert grid == row["polytopes"], (grid, row["polytopes"])
        row["kernel_us_rocprofv3"] = us
        row["kernel_us_per_polytope"] = us / row["polytopes"]
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    raise SystemExit(0)

import ctypes as C  # noqa: E402
from concurrent.futures import ThreadPoolExecutor  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

from frx_import import frx  # noqa: E402
from fast_racing_amd import scenario as sc  # noqa: E402
import corridor_states as cs  # noqa: E402

torch.cuda.init()                         # torch's HIP runtime first, then the library's (the order bench.py keeps)
if frx.lib().frx_device_count() < 1:
    raise SystemExit("enumerate_throughput.py needs a HIP device")


def host_time(polys, threads):
    """seconds for frx_enumerate_vertices over polys (record arrays) on `threads` threads"""
    L = frx.lib()
    flat = [np.ascontiguousarray(p).reshape(-1) for p in polys]

    def work(chunk):
        nv = C.c_int(); out = np.zeros(3 * 512)
        for r in chunk:
            L.frx_enumerate_vertices(len(r) // 6, r, out.ctypes.data, 512, C.byref(nv))
    chunks = [flat[i::threads] for i in range(threads)]
    t0 = time.perf_counter()
    if threads == 1:
        work(chunks[0])
    else:
        with ThreadPoolExecutor(threads) as ex:
            list(ex.map(work, chunks))
    return time.perf_counter() - t0


rows = []
stream = torch.cuda.current_stream().cuda_stream
routes = [cs.route(sc, s, g) for s, g in cs.WORLD_SEEDS][:args.base_routes]
for n_obs in [int(p) for p in args.points.split(",")]:
    cloud = cs.cloud_around(np.random.default_rng(n_obs), routes, n_obs)
    base = [[np.ascontiguousarray(H.T) for H in frx.corridor_generate(p, cloud, cs.BBOX, cs.MAP_HEIGHT, cs.MAX_SEG)] for p in routes]
    for B in [int(b) for b in args.routes.split(",")]:
        rng = np.random.default_rng(B)
        cells = []; coarse_n = []
        for b in range(B):
            shift = np.concatenate([np.zeros(3), rng.uniform(-5.0, 5.0, 3)]) if b >= len(base) else np.zeros(6)
            corridor = base[b % len(base)]
            cells += [rec + shift for rec in corridor]; coarse_n.append(len(corridor))
        coarse_n = np.array(coarse_n, np.int32)
        h_off = np.zeros(len(cells) + 1, np.int32); h_off[1:] = np.cumsum([len(c) for c in cells]); h_rec = np.concatenate(cells).reshape(-1)
        tasks = []; polys = []; m = 0
        for n in coarse_n:
            for i in range(n):
                tasks.append([h_off[m + i], h_off[m + i + 1] - h_off[m + i], 0, 0]); polys.append(h_rec[6 * h_off[m + i]:6 * h_off[m + i + 1]])
                if i + 1 < n:
                    tasks.append([h_off[m + i], h_off[m + i + 1] - h_off[m + i], h_off[m + i + 1], h_off[m + i + 2] - h_off[m + i + 1]])
                    polys.append(h_rec[6 * h_off[m + i]:6 * h_off[m + i + 2]])
            m += n
        tasks = np.array(tasks, np.int32); NT = len(tasks); K = tasks[:, 1] + tasks[:, 3]
        d_tasks = torch.from_numpy(tasks.reshape(-1)).cuda(); d_rec = torch.from_numpy(h_rec).cuda()
        d_slot = torch.zeros(NT * args.cap_v * 3, dtype=torch.float64, device="cuda"); d_nv = torch.zeros(NT, dtype=torch.int32, device="cuda")
        d_st = torch.zeros(NT, dtype=torch.int32, device="cuda")

        def launch():
            frx.enumerate_vertices_batch_device(NT, d_tasks.data_ptr(), d_rec.data_ptr(), args.cap_v, d_slot.data_ptr(), d_nv.data_ptr(), d_st.data_ptr(), stream)
        launch()
        torch.cuda.synchronize()
        nv, status = d_nv.cpu().numpy(), d_st.cpu().numpy()
        row = dict(routes=B, points=n_obs, polytopes=NT, K_min=int(K.min()), K_median=float(np.median(K)), K_max=int(K.max()), triples=int((K * (K - 1) * (K - 2) // 6).sum()),
                   vertices_median=float(np.median(nv)), vertices_max=int(nv.max()), status_not_ok=int((status != 0).sum()))
        if not args.kernel_only:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.reps):
                launch()
            e1.record()
            torch.cuda.synchronize()
            row["device_launch_ms"] = e0.elapsed_time(e1) / args.reps
            frx.enumerate_vertices_batch(coarse_n, h_off, h_rec, cap_v=args.cap_v)
            t0 = time.perf_counter()
            v_off, v_rec, st = frx.enumerate_vertices_batch(coarse_n, h_off, h_rec, cap_v=args.cap_v)
            row["blocking_call_ms"] = (time.perf_counter() - t0) * 1e3
            assert np.array_equal(st, status) and np.array_equal(np.diff(v_off), nv)
            nh = min(NT, args.host_polys)
            if nh:
                pick = np.random.default_rng(1).permutation(NT)[:nh]
                sub = [polys[i] for i in pick]
                scale = float((K.astype(np.float64) ** 4).sum() / (K[pick].astype(np.float64) ** 4).sum())      # the host's cost grows as K^4: weigh the sample
                t1 = host_time(sub, 1); tN = host_time(sub, args.threads)
                row.update(host_polytopes_measured=nh, host_extrapolated=bool(nh < NT), host_us_per_polytope_1_thread=t1 * 1e6 / nh,
                           host_ms_batch_1_thread=t1 * 1e3 * scale, host_ms_batch_pool=tN * 1e3 * scale, host_pool_threads=args.threads,
                           speedup_device_launch_over_pool=tN * 1e3 * scale / row["device_launch_ms"],
                           speedup_blocking_call_over_pool=tN * 1e3 * scale / row["blocking_call_ms"])
        rows.append(row)
        print(json.dumps(row), flush=True)
res = dict(what="frx_enumerate_vertices_batch throughput against frx_enumerate_vertices on the host", cap_v=args.cap_v, base_routes=len(routes), rows=rows)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
