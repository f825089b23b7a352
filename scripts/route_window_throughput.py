#!/usr/bin/env python3
"""Throughput of the route batch searched inside per-leg windows (frx_route_plan_window_batch_device, csrc/frx_route_window_kernel.hpp) next to the whole-map
form (frx_route_plan_batch_device, csrc/frx_route_kernel.hpp) on one box in one run.  Fills the table of DESIGN 3.23 and writes
profiles/route_window_throughput.json.

Part 1: the batches of DESIGN 3.21 - 1, 32 and 512 routes through 3 gates (4 legs each) on the 160 x 460 x 27 pillar map, drawn as scripts/route_throughput.py
draws them - through the whole-map form and through the window form at pads of 10, 20 and 40 cells.  cap_window is the largest window the host form reports at
that pad.  Part 2: a map of 700 x 4000 x 28 cells (70 x 400 x 2.8 m at 0.1 m) with pillars at the same density, 512 routes of four legs with gates 10 to 15 m
apart, pad 20: a batch whose whole-map labels would take 160 GB.
Per row: the launch interval (the median of --reps single launches, each between two HIP events, after one warm-up launch), the workspace, the share of legs
with status 0, 6 and 7, and whether the device's outputs are the host form's bit for bit."""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ap = argparse.ArgumentParser()
ap.add_argument("--batches", default="1,32,512")
ap.add_argument("--pads", default="10,20,40")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--cap-level", type=int, default=16384)
ap.add_argument("--cap-raw", type=int, default=2048)
ap.add_argument("--cap-pts", type=int, default=1024)
ap.add_argument("--large-routes", type=int, default=512, help="routes of the 700 x 4000 x 28 case; 0 skips it")
ap.add_argument("--large-pad", type=int, default=20)
ap.add_argument("--out", default="profiles/route_window_throughput.json")
args = ap.parse_args()
if args.reps < 5:
    raise SystemExit("a timing is a median of at least five launches")

import numpy as np  # noqa: E402
from frx_import import frx  # noqa: E402

if frx.lib().frx_device_count() < 1:
    raise SystemExit("route_window_throughput.py needs a HIP device")
H = None
for name in ("libamdhip64.so", "libamdhip64.so.7"):                       # the runtime libfrx.so is linked to, by its plain name first
    try:
        H = C.CDLL(name)
        break
    except OSError:
        pass
if H is None:
    raise SystemExit("route_window_throughput.py: cannot load the HIP runtime")


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


def median_ms(launch, reps):
    launch()                                                              # warm-up
    check(H.hipDeviceSynchronize())
    e0, e1 = C.c_void_p(), C.c_void_p()
    check(H.hipEventCreate(C.byref(e0))); check(H.hipEventCreate(C.byref(e1)))
    times = []
    for _ in range(reps):
        check(H.hipEventRecord(e0, None))
        launch()
        check(H.hipEventRecord(e1, None))
        check(H.hipEventSynchronize(e1))
        ms = C.c_float()
        check(H.hipEventElapsedTime(C.byref(ms), e0, e1))
        times.append(ms.value)
    H.hipEventDestroy(e0); H.hipEventDestroy(e1)
    return float(np.median(times)), [float(t) for t in times]


def pillar_map(x_size, y_size, nz, n_pillars, y_range, x_half, seed=11):
    """the map of MapUtil::setParam's origin with nz layers of 0.1 m and pillars 2.2 m apart or more"""
    rng = np.random.default_rng(seed)
    vm = frx.VoxelMap([-x_size / 2, -10.0, 0.0], [int(round(x_size / 0.1)), int(round(y_size / 0.1)), nz], 0.1)
    pillars = np.zeros((0, 2))
    while len(pillars) < n_pillars:
        c = np.array([rng.uniform(-x_half, x_half), rng.uniform(*y_range)])
        if not len(pillars) or (np.linalg.norm(pillars - c, axis=1) > 2.2).all():
            pillars = np.vstack([pillars, c])
    d = np.arange(-0.3, 0.31, 0.1)
    col = np.array([[dx, dy, z] for dx in d for dy in d for z in np.arange(0.05, 2.8, 0.1)])
    cloud = (np.concatenate([pillars, np.zeros((len(pillars), 1))], axis=1)[:, None, :] + col[None, :, :]).reshape(-1, 3)
    vm.mark_cloud(cloud)
    return vm, pillars, rng


def clear(p, pillars):
    return (np.linalg.norm(pillars - p[:2], axis=1) > 1.2).all()


def draw_route(rng, pillars):
    """the route of scripts/route_throughput.py: start, three gates, goal along y"""
    def clear_point(y):
        while True:
            p = np.array([rng.uniform(-5, 5), y + rng.uniform(-1, 1), rng.uniform(1.0, 2.0)])
            if clear(p, pillars):
                return p
    return np.array([clear_point(-8.0)] + [clear_point(y) for y in (3.0, 13.0, 24.0)] + [clear_point(34.0)])


def draw_long_route(rng, pillars, x_half, y_range):
    """five waypoints, each 10 to 15 m from the one before it, within 30 degrees of +y"""
    while True:
        p = np.array([rng.uniform(-x_half, x_half), rng.uniform(y_range[0], y_range[1] - 65.0), rng.uniform(1.0, 2.0)])
        if clear(p, pillars):
            break
    wp = [p]
    while len(wp) < 5:
        a, d = rng.uniform(-np.pi / 6, np.pi / 6), rng.uniform(10.0, 15.0)
        q = np.array([wp[-1][0] + d * np.sin(a), wp[-1][1] + d * np.cos(a), rng.uniform(1.0, 2.0)])
        if abs(q[0]) <= x_half and clear(q, pillars):
            wp.append(q)
    return np.array(wp)


def shares(status):
    n = max(len(status), 1)
    return {str(s): float((status == s).sum()) / n for s in (0, 6, 7)}


def run(vm, routes, pad, label):
    """one row: pad None is the whole-map form"""
    B = len(routes)
    off, pts = frx.pack_routes(routes)
    NL = int(off[-1]) - B
    cap_total = NL * args.cap_pts
    caps = dict(cap_level=args.cap_level, cap_raw=args.cap_raw, cap_pts=args.cap_pts, cap_total=cap_total)
    row = dict(case=label, routes=B, legs=NL, pad=pad, reps=args.reps)
    if pad is None:
        nbytes = frx.route_search_workspace(vm.dim, NL, args.cap_level, args.cap_raw, args.cap_pts)
        ref = None
    else:
        t0 = time.perf_counter()
        ref = vm.route_batch_window_host(routes, pad, (1 << 31) - 4, **caps)
        row["host_form_1_thread_ms"] = (time.perf_counter() - t0) * 1e3
        sizes = ref["leg_window"][:, 3:6].astype(np.int64).prod(axis=1)
        cap_window = int(sizes.max())
        nbytes = frx.route_window_workspace(NL, args.cap_level, args.cap_raw, args.cap_pts, cap_window)
        row.update(cap_window=cap_window, median_window_cells=int(np.median(sizes[sizes > 0])) if (sizes > 0).any() else 0)
    row["workspace_bytes"] = nbytes
    bufs = dict(cells=Dev(vm.cells.size, vm.cells), off=Dev(off.nbytes, off), pts=Dev(pts.nbytes, pts), work=Dev(nbytes), path_off=Dev(4 * (B + 1)),
                path=Dev(24 * cap_total), rst=Dev(4 * B), lst=Dev(4 * NL), lev=Dev(4 * NL), mx=Dev(4 * NL), win=Dev(32 * NL))
    ms = vm.device_struct(bufs["cells"].p)
    if pad is None:
        def launch():
            frx.route_plan_batch_device(ms, B, NL, bufs["off"].p, bufs["pts"].p, args.cap_level, args.cap_raw, args.cap_pts, cap_total, bufs["work"].p,
                                        bufs["path_off"].p, bufs["path"].p, bufs["rst"].p, bufs["lst"].p, bufs["lev"].p, bufs["mx"].p)
    else:
        def launch():
            frx.route_plan_window_batch_device(ms, B, NL, bufs["off"].p, bufs["pts"].p, pad, cap_window, args.cap_level, args.cap_raw, args.cap_pts, cap_total,
                                               bufs["work"].p, bufs["path_off"].p, bufs["path"].p, bufs["rst"].p, bufs["lst"].p, bufs["lev"].p, bufs["mx"].p,
                                               bufs["win"].p)
    row["device_launch_ms"], row["device_launch_all_ms"] = median_ms(launch, args.reps)
    dev = dict(path_off=bufs["path_off"].get(np.int32), leg_status=bufs["lst"].get(np.int32), levels=bufs["lev"].get(np.int32),
               max_level_cells=bufs["mx"].get(np.int32), route_status=bufs["rst"].get(np.int32), leg_window=bufs["win"].get(np.int32).reshape(-1, 8))
    dev["path"] = bufs["path"].get(np.float64)[:3 * dev["path_off"][-1]].reshape(-1, 3)
    for d in bufs.values():
        d.close()
    row["leg_status_share"] = shares(dev["leg_status"])
    row["routes_whole"] = int((dev["route_status"] == 0).sum())
    ok = dev["leg_status"] == 0
    row["deepest_level"] = int(dev["levels"].max())
    row["largest_level_cells"] = int(dev["max_level_cells"].max())
    if ref is not None:
        row["bit_identical_to_host_form"] = bool(all(np.array_equal(np.asarray(dev[k]).view(np.uint8), np.asarray(ref[k]).view(np.uint8))
                                                     for k in ("path", "path_off", "leg_status", "levels", "max_level_cells", "route_status", "leg_window")))
    print(json.dumps(row), flush=True)
    return row, dev, ok


rows = []
vm, pillars, rng = pillar_map(16.0, 46.0, 27, 45, (-6, 32), 7)
all_routes = [draw_route(rng, pillars) for _ in range(max(int(b) for b in args.batches.split(",")))]
for B in [int(b) for b in args.batches.split(",")]:
    whole_row, whole, _ = run(vm, all_routes[:B], None, "pillar map 160 x 460 x 27")
    rows.append(whole_row)
    for pad in [int(p) for p in args.pads.split(",")]:
        row, dev, ok = run(vm, all_routes[:B], pad, "pillar map 160 x 460 x 27")
        # a certified leg is the whole-map leg: its level, and - for routes whole in both - every point
        row["certified_levels_equal_whole_map"] = bool(np.array_equal(dev["levels"][ok], whole["levels"][ok]) and (whole["leg_status"][ok] == 0).all())
        same_routes = [r for r in range(B) if dev["route_status"][r] == 0]
        row["whole_routes_equal_whole_map"] = bool(all(np.array_equal(dev["path"][dev["path_off"][r]:dev["path_off"][r + 1]].view(np.uint8),
                                                                      whole["path"][whole["path_off"][r]:whole["path_off"][r + 1]].view(np.uint8)) for r in same_routes))
        rows.append(row)
if args.large_routes > 0:
    t0 = time.perf_counter()
    density = 45 / (16.0 * 46.0)
    big, big_pillars, rng = pillar_map(70.0, 400.0, 28, int(round(density * 70.0 * 400.0)), (-9.0, 389.0), 34.0, seed=12)
    print(json.dumps(dict(large_map_dim=[int(d) for d in big.dim], pillars=len(big_pillars), built_s=time.perf_counter() - t0)), flush=True)
    long_routes = [draw_long_route(rng, big_pillars, 32.0, (-9.0, 389.0)) for _ in range(args.large_routes)]
    row, dev, ok = run(big, long_routes, args.large_pad, "map 700 x 4000 x 28")
    n_cells = int(np.prod(big.dim))
    row["whole_map_label_bytes_for_this_batch"] = int(row["legs"]) * ((n_cells + 3) // 4 * 4)
    rows.append(row)

res = dict(what="frx_route_plan_window_batch_device next to frx_route_plan_batch_device: launch intervals (median of single launches), workspaces and certified shares",
           caps=dict(cap_level=args.cap_level, cap_raw=args.cap_raw, cap_pts=args.cap_pts), rows=rows)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
