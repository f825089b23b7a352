#!/usr/bin/env python3
"""Throughput of the voxel map's distance field on the device (frx_map_esdf_device, csrc/frx_esdf_kernel.hpp) and of the screen of a batch against it
(frx_trajectory_map_distance, csrc/frx_mapdist_kernel.hpp).  Fills the table of DESIGN 3.20.

Field builds: the 70 x 400 x 2.8 m Zhangjiajie volume at 0.1 m (700 x 4000 x 28 cells) and at 0.2 m (350 x 2000 x 14), each marked on the device from clouds of
4 096 and 65 536 points spread evenly over the volume, and left empty - without an occupied cell every search of the baseline would walk its whole line, which
is what the "line has a site" flags are for.  Per case: the device form's launch interval (HIP events round back-to-back calls on one stream: five kernels), the
blocking call and frx_map_esdf on one host thread (host clock), and the bytes the passes must move - per cell 2 + 16 in the z pass (the cells twice, dz^2 of both
site sets written and read back; the second write only where the sweep down is closer), 8 + 8 in the y pass, 8 + 24 in the x pass - against the HBM peak of
8 TB/s.  The device's three fields are compared with the host's, bit for bit, in the same run.

Screens: 1 x 64, 32 x 64 and 512 x 64 pieces at the initial guess, M = 256, against pos of the 0.1 m volume with the 65 536-point cloud: the screen's launch
interval next to frx_trajectory_clearance's (k_traj_clear) for the same batch and cloud.

Kernel times per pass come from a run of their own under the profiler's kernel trace, never from this process's clocks:
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python scripts/esdf_throughput.py --trace
    python scripts/esdf_throughput.py --merge-trace <dir> --out profiles/esdf_throughput.json
--trace launches every field case three times in a fixed order and nothing else; --merge-trace reads the dispatches back in that order (no device needed) and
adds the median per pass to the JSON the timing run wrote.
"""
import argparse
import ctypes as C
import csv
import glob
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ap = argparse.ArgumentParser()
ap.add_argument("--maps", default="700x4000x28,350x2000x14")
ap.add_argument("--clouds", default="4096,65536,0")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--batches", default="1,32,512")
ap.add_argument("--intervals", type=int, default=256)
ap.add_argument("--no-host", action="store_true", help="skip frx_map_esdf on the host thread (and with it the comparison)")
ap.add_argument("--no-screens", action="store_true")
ap.add_argument("--trace", action="store_true", help="the profiler's run: every field case three times, nothing else")
ap.add_argument("--merge-trace", default="", help="directory of a rocprofv3 --kernel-trace run of --trace: add kernel ms per pass to --out")
ap.add_argument("--out", default="", help="write (or, with --merge-trace, update) the JSON result here")
args = ap.parse_args()

import numpy as np  # noqa: E402

HBM_PEAK = 8.0e12
TRACE_RUNS = 3
PASSES = ("k_esdf_flags", "k_esdf_z", "k_esdf_ycol", "k_esdf_y", "k_esdf_x")      # (a name is matched in this order: k_esdf_ycol before k_esdf_y)
maps = [tuple(int(v) for v in m.split("x")) for m in args.maps.split(",")]
clouds = [int(c) for c in args.clouds.split(",")]
cases = [(dim, n) for dim in maps for n in clouds]


def merge_trace():
    files = glob.glob(os.path.join(args.merge_trace, "**", "*kernel_trace.csv"), recursive=True)
    if len(files) != 1:
        raise SystemExit(f"expected one kernel trace under {args.merge_trace}, found {files}")
    rows = []
    with open(files[0]) as f:
        for r in csv.DictReader(f):
            name = next((p for p in PASSES if p in r["Kernel_Name"]), None)
            if name:
                rows.append((int(r["Start_Timestamp"]), name, (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6))
    rows.sort()
    if len(rows) != len(cases) * TRACE_RUNS * len(PASSES):
        raise SystemExit(f"{len(rows)} dispatches of the passes in the trace, {len(cases) * TRACE_RUNS * len(PASSES)} expected")
    res = json.load(open(args.out))
    for k, (dim, n) in enumerate(cases):
        mine = rows[k * TRACE_RUNS * len(PASSES):(k + 1) * TRACE_RUNS * len(PASSES)]
        row = next(r for r in res["fields"] if tuple(r["dim"]) == dim and r["cloud_points"] == n)
        ms = {p: float(np.median([t for _, name, t in mine[len(PASSES):] if name == p])) for p in PASSES}      # (the first run of a case is its warm-up)
        row["kernel_ms"] = ms
        row["kernel_ms_total"] = sum(ms.values())
        row["share_of_hbm_peak"] = row["bytes_moved"] / HBM_PEAK / (row["kernel_ms_total"] * 1e-3)
    json.dump(res, open(args.out, "w"), indent=1)
    print(json.dumps(res["fields"]))


if args.merge_trace:
    merge_trace()
    sys.exit(0)

from frx_import import frx  # noqa: E402
from fast_racing_amd import scenario as sc  # noqa: E402

if frx.lib().frx_device_count() < 1:
    raise SystemExit("esdf_throughput.py needs a HIP device")
H = C.CDLL("libamdhip64.so.7")
ORIGIN = (-35.0, -10.0, 0.0)
EXTENT = (70.0, 400.0, 2.8)


def check(rc):
    if rc != 0:
        raise SystemExit(f"HIP error {rc}")


class Dev:
    def __init__(self, nbytes, host=None):
        self.n = int(nbytes)
        self.ptr = C.c_void_p()
        check(H.hipMalloc(C.byref(self.ptr), C.c_size_t(max(self.n, 8))))
        if host is not None:
            check(H.hipMemcpy(self.ptr, C.c_void_p(host.ctypes.data), C.c_size_t(self.n), 1))
        else:
            check(H.hipMemset(self.ptr, 0, C.c_size_t(max(self.n, 8))))

    @property
    def p(self):
        return self.ptr.value

    def get(self, dtype):
        out = np.empty(self.n // np.dtype(dtype).itemsize, dtype)
        check(H.hipDeviceSynchronize())
        check(H.hipMemcpy(C.c_void_p(out.ctypes.data), self.ptr, C.c_size_t(self.n), 2))
        return out

    def close(self):
        H.hipFree(self.ptr)


def interval_ms(launch, reps):
    launch()
    check(H.hipDeviceSynchronize())
    e0, e1 = C.c_void_p(), C.c_void_p()
    check(H.hipEventCreate(C.byref(e0))); check(H.hipEventCreate(C.byref(e1)))
    check(H.hipEventRecord(e0, None))
    for _ in range(reps):
        launch()
    check(H.hipEventRecord(e1, None))
    check(H.hipEventSynchronize(e1))
    ms = C.c_float()
    check(H.hipEventElapsedTime(C.byref(ms), e0, e1))
    H.hipEventDestroy(e0); H.hipEventDestroy(e1)
    return ms.value / reps


def marked_map(dim, n_pts):
    """the volume at dim cells, its cloud, and the cells marked on the device"""
    res = EXTENT[0] / dim[0]
    vmap = frx.VoxelMap(ORIGIN, dim, res)
    pts = np.random.default_rng(n_pts + dim[0]).uniform(np.array(ORIGIN), np.array(ORIGIN) + np.array(EXTENT), (n_pts, 3))
    cells = Dev(vmap.cells.size)
    if n_pts:
        dp, cnt = Dev(pts.nbytes, pts), Dev(4)
        frx.map_mark_cloud_device(vmap.device_struct(cells.p), cells.p, n_pts, dp.p, cnt.p)
        inside = int(cnt.get(np.int32)[0])
        dp.close(); cnt.close()
    else:
        inside = 0
    return vmap, pts, cells, inside


fields = []
for dim, n_pts in cases:
    n = dim[0] * dim[1] * dim[2]
    vmap, pts, cells, inside = marked_map(dim, n_pts)
    work = Dev(frx.map_esdf_workspace(dim))
    out = [Dev(8 * n) for _ in range(3)]
    ms = vmap.device_struct(cells.p)

    def launch():
        frx.map_esdf_device(ms, out[0].p, out[1].p, out[2].p, work.p)
    if args.trace:
        for _ in range(TRACE_RUNS):
            launch()
            check(H.hipDeviceSynchronize())
    else:
        dev_ms = interval_ms(launch, args.reps)
        vmap.cells[:] = cells.get(np.int8)
        occupied = int((vmap.cells > 0).sum())
        vmap.esdf_on_device()
        t0 = time.perf_counter()
        blk = vmap.esdf_on_device()
        blk_ms = (time.perf_counter() - t0) * 1e3
        row = dict(dim=list(dim), res=vmap.res, cells=n, cloud_points=n_pts, points_inside=inside, occupied_cells=occupied, reps=args.reps,
                   device_launch_ms=dev_ms, blocking_call_ms=blk_ms, bytes_moved=66 * n, workspace_bytes=work.n)
        if not args.no_host:
            t0 = time.perf_counter()
            host = vmap.esdf()
            row["host_thread_ms"] = (time.perf_counter() - t0) * 1e3
            row["bit_identical_to_host"] = bool(all(np.array_equal(out[i].get(np.float64).view(np.uint64), host[k].view(np.uint64)) and
                                                    np.array_equal(blk[k].view(np.uint64), host[k].view(np.uint64)) for i, k in enumerate(("pos", "neg", "all"))))
            del host
        del blk
        fields.append(row)
        print(json.dumps(row), flush=True)
    for d in [cells, work] + out:
        d.close()

if args.trace:
    sys.exit(0)

screens = []
if not args.no_screens:
    _, N, gates, kappa = sc.CONFIGS["headline"]
    M, n_obs = args.intervals, 65536
    vmap, pts, cells, _ = marked_map(maps[0], n_obs)
    n = vmap.cells.size
    work, pos = Dev(frx.map_esdf_workspace(maps[0])), Dev(8 * n)
    ms = vmap.device_struct(cells.p)
    frx.map_esdf_device(ms, pos.p, 0, 0, work.p)
    check(H.hipDeviceSynchronize())
    work.close()
    obs = Dev(pts.nbytes, pts)
    for B in [int(b) for b in args.batches.split(",")]:
        cands = sc.make_batch(0, B, N, gates) if B <= 32 else [sc.make_candidate(b, N, gates) for b in range(B)]
        prob = frx.Problem(cands, sc.ZHANGJIAJIE, qd_intervals=kappa)
        T, Cf = prob.forward(prob.initial_guess())
        Cf = np.ascontiguousarray(Cf).reshape(-1)
        Td, Cd, rows = Dev(T.nbytes, np.ascontiguousarray(T)), Dev(Cf.nbytes, Cf), Dev(32 * prob.P)
        us_screen = 1e3 * interval_ms(lambda: prob.trajectory_map_distance_device(Td.p, Cd.p, ms, pos.p, rows.p, M), 20)
        r = rows.get(np.float64).reshape(-1, 4)
        wbytes = prob.trajectory_clearance_workspace(n_obs, M)
        wd, crow = Dev(max(wbytes, 8)), Dev(32 * prob.P)
        us_clear = 1e3 * interval_ms(lambda: prob.trajectory_clearance_device(Td.p, Cd.p, obs.p, n_obs, wd.p if wbytes else 0, crow.p, M), 1 if prob.P > 4096 else 3)
        c = crow.get(np.float64).reshape(-1, 4)
        screens.append(dict(batch=B, pieces=prob.P, intervals=M, lookups=prob.P * (M + 1), cloud_points=n_obs, screen_launch_us=us_screen, clearance_launch_us=us_clear,
                            samples_outside=int(r[:, 3].sum()), smallest_dist=float(r[:, 0].min()), smallest_clear_dist=float(c[:, 1].min()),
                            largest_gap_to_clear_dist=float(np.abs(r[:, 0] - c[:, 1]).max()), bound=float(np.sqrt(3.0) * vmap.res + 1e-9)))
        print(json.dumps(screens[-1]), flush=True)
        for d in (Td, Cd, rows, wd, crow):
            d.close()
        prob.close()

res = dict(what="frx_map_esdf_device and frx_trajectory_map_distance throughput (one synthetic scenario: clouds spread evenly over the Zhangjiajie volume)",
           hbm_peak_bytes_per_s=HBM_PEAK, fields=fields, screens=screens)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
