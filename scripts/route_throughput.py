#!/usr/bin/env python3
"""Throughput of the route batch on the device (frx_route_plan_batch[_device], csrc/frx_route_kernel.hpp) next to the host search of the same routes.  Fills the
table of DESIGN 3.21 and writes profiles/route_throughput.json.

Cases: 1, 32 and 512 routes through 3 gates (4 legs each) on the 160 x 460 x 27 pillar map of tests/test_front_end.py::test_voxel_map_to_trajectory_on_the_device;
every route draws its own start, gates and goal the way that test draws its one route.  Columns per case:
  device_launch_ms   the device form's launch interval (HIP events round back-to-back calls on one stream: four kernels)
  blocking_call_ms   frx_route_plan_batch on host pointers (upload of map and waypoints, workspace allocation, the launches, download; host clock)
  host_1_thread_ms   frx_route_plan, one call per route, legs on one thread (host clock)
  host_16_threads_ms the same routes, 16 at a time on a thread pool, each call on one thread (the calls release the interpreter lock)
The host columns are the yardstick: the reference's own search, A* with eps = 1.  It returns another shortest path than the level search, so the device's routes are
compared with frx_route_plan_levels_batch (bit for bit); tests/test_route_levels_cpu.py holds the two searches to the same length.  --host-routes limits the host columns to the
first so many routes of a case (the JSON says how many were run; a column that was not run is "unmeasured")."""
import argparse
import ctypes as C
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ap = argparse.ArgumentParser()
ap.add_argument("--batches", default="1,32,512")
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--host-routes", type=int, default=512)
ap.add_argument("--threads", type=int, default=16)
ap.add_argument("--cap-level", type=int, default=16384)
ap.add_argument("--cap-raw", type=int, default=2048)
ap.add_argument("--cap-pts", type=int, default=1024)
ap.add_argument("--out", default="profiles/route_throughput.json")
args = ap.parse_args()

import numpy as np  # noqa: E402
from frx_import import frx  # noqa: E402

if frx.lib().frx_device_count() < 1:
    raise SystemExit("route_throughput.py needs a HIP device")
H = None
for name in ("libamdhip64.so", "libamdhip64.so.7"):                       # the runtime libfrx.so is linked to, by its plain name first
    try:
        H = C.CDLL(name)
        break
    except OSError:
        pass
if H is None:
    raise SystemExit("route_throughput.py: cannot load the HIP runtime")


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


def pillar_map():
    rng = np.random.default_rng(11)
    vm = frx.VoxelMap.from_params(16.0, 46.0, 2.8, 0.1)
    pillars = []
    while len(pillars) < 45:
        c = np.array([rng.uniform(-7, 7), rng.uniform(-6, 32)])
        if all(np.linalg.norm(c - q) > 2.2 for q in pillars):
            pillars.append(c)
    cloud = np.array([[c[0] + dx, c[1] + dy, z] for c in pillars for dx in np.arange(-0.3, 0.31, 0.1) for dy in np.arange(-0.3, 0.31, 0.1)
                      for z in np.arange(0.05, 2.8, 0.1)])
    vm.mark_cloud(cloud)
    return vm, pillars, rng


def draw_route(rng, pillars):
    def clear_point(y):
        while True:
            p = np.array([rng.uniform(-5, 5), y + rng.uniform(-1, 1), rng.uniform(1.0, 2.0)])
            if all(np.linalg.norm(p[:2] - q) > 1.2 for q in pillars):
                return p
    return np.array([clear_point(-8.0)] + [clear_point(y) for y in (3.0, 13.0, 24.0)] + [clear_point(34.0)])


vm, pillars, rng = pillar_map()
all_routes = [draw_route(rng, pillars) for _ in range(max(int(b) for b in args.batches.split(",")))]
rows = []
for B in [int(b) for b in args.batches.split(",")]:
    routes = all_routes[:B]
    off, pts = frx.pack_routes(routes)
    NL = int(off[-1]) - B
    cap_total = NL * args.cap_pts
    nbytes = frx.route_search_workspace(vm.dim, NL, args.cap_level, args.cap_raw, args.cap_pts)
    bufs = dict(cells=Dev(vm.cells.size, vm.cells), off=Dev(off.nbytes, off), pts=Dev(pts.nbytes, pts), work=Dev(nbytes), path_off=Dev(4 * (B + 1)),
                path=Dev(24 * cap_total), rst=Dev(4 * B), lst=Dev(4 * NL), lev=Dev(4 * NL), mx=Dev(4 * NL))
    ms = vm.device_struct(bufs["cells"].p)

    def launch():
        frx.route_plan_batch_device(ms, B, NL, bufs["off"].p, bufs["pts"].p, args.cap_level, args.cap_raw, args.cap_pts, cap_total, bufs["work"].p,
                                    bufs["path_off"].p, bufs["path"].p, bufs["rst"].p, bufs["lst"].p, bufs["lev"].p, bufs["mx"].p)
    dev_ms = interval_ms(launch, args.reps)
    dev = dict(path_off=bufs["path_off"].get(np.int32), leg_status=bufs["lst"].get(np.int32), levels=bufs["lev"].get(np.int32), max_level=bufs["mx"].get(np.int32),
               route_status=bufs["rst"].get(np.int32))
    dev["path"] = bufs["path"].get(np.float64)[:3 * dev["path_off"][-1]].reshape(-1, 3)
    for d in bufs.values():
        d.close()
    caps = dict(cap_level=args.cap_level, cap_raw=args.cap_raw, cap_pts=args.cap_pts, cap_total=cap_total)
    vm.route_batch(routes, **caps)
    t0 = time.perf_counter()
    blk = vm.route_batch(routes, **caps)
    blk_ms = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    ref = vm.route_batch_host(routes, **caps)
    levels_host_ms = (time.perf_counter() - t0) * 1e3
    same = all(np.array_equal(np.asarray(a).view(np.uint8), np.asarray(b).view(np.uint8)) for a, b in
               [(dev["path"], ref["path"]), (blk["path"], ref["path"]), (dev["path_off"], ref["path_off"]), (dev["leg_status"], ref["leg_status"]),
                (dev["levels"], ref["levels"]), (dev["max_level"], ref["max_level_cells"]), (dev["route_status"], ref["route_status"])])
    row = dict(routes=B, legs=NL, reps=args.reps, workspace_bytes=nbytes, device_launch_ms=dev_ms, blocking_call_ms=blk_ms, levels_host_1_thread_ms=levels_host_ms,
               bit_identical_to_levels_host=bool(same), legs_ok=int((ref["leg_status"] == 0).sum()), deepest_level=int(ref["levels"].max()),
               largest_level_cells=int(ref["max_level_cells"].max()), route_points=int(ref["path_off"][-1]),
               host_1_thread_ms="unmeasured", host_16_threads_ms="unmeasured", host_routes=0, host_legs_all_ok="unmeasured")
    n_host = min(B, args.host_routes)
    if n_host > 0:
        def one(wp):
            return vm.route(wp[0], wp[-1], wp[1:-1], eps=1.0, use_jps=False, threads=1)
        t0 = time.perf_counter()
        host = [one(wp) for wp in routes[:n_host]]
        row["host_1_thread_ms"] = (time.perf_counter() - t0) * 1e3
        with ThreadPoolExecutor(args.threads) as pool:
            t0 = time.perf_counter()
            list(pool.map(one, routes[:n_host]))
            row["host_16_threads_ms"] = (time.perf_counter() - t0) * 1e3
        row["host_routes"] = n_host
        row["host_legs_all_ok"] = bool(all((st == 0).all() for _, st, _ in host))
    rows.append(row)
    print(json.dumps(row), flush=True)

res = dict(what="frx_route_plan_batch[_device] throughput: routes through 3 gates on the 160 x 460 x 27 pillar map, next to frx_route_plan on the same machine",
           host_threads=args.threads, caps=dict(cap_level=args.cap_level, cap_raw=args.cap_raw, cap_pts=args.cap_pts), rows=rows)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
