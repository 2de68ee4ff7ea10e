#!/usr/bin/env python3
"""Timing of range data into many resident TSDF2D grids: one cmx_tsdf2d_insert_batch call against
the same insertions as single cmx_tsdf2d_insert calls; prints one JSON line and writes it to --out.

The grids have the benchmark submap's limits (400 x 400 at 0.05 m, all unknown at first), the
scans are ~1000 rays from free poses of its room, transformed into the map frame: no grid grows,
so every repeat does the same work.  Options: trajectory_builder_2d.lua's with update_free_space
on.  Cases:
  robots_1, robots_16, robots_64   N robots x 2 grids: each robot's scan goes into both of its
                                   grids by the same pointers (ActiveSubmaps2D::InsertRangeData)
  grids_64_rounds_8                64 grids x 8 scans each, grid after grid in the list
Legs per case (median, min and max over --repeats after --warmup, host clock; every device call
ends in a synchronise; the argument arrays are built once, outside the clock):
  batch_ms          one cmx_tsdf2d_insert_batch call for the whole list
  single_calls_ms   one cmx_tsdf2d_insert call per insertion, in list order, into grids of their own
  plan_ms           cmx_debug_tsdf2d_insert_plan alone: the host's share of the batch call (sort,
                    normals, weights per distinct scan, ray ends per insertion; no device)
and `batch_equals_single_calls`: limits and both planes of every grid afterwards.
--library PATH loads another build of the library (the parent commit's, for the yardstick of
single_calls_ms on the same box); the batch and plan legs are left out where the entry point is
missing.
--yardstick F [F ...] takes such runs' JSON (before and after this one, same box) and records
their figures, their spread and the ratios to this run's; with --merge F nothing is measured: F
is an earlier run of this tree, to which the yardsticks are added.
--time-limit S ends the process after S seconds whatever it is doing.
Writes profiles/tsdf2d_insert_batch_timing.json unless --out names another file.
Usage: python tools/tsdf2d_insert_batch_timing.py [--repeats 20] [--warmup 3] [--library PATH]
                                                  [--yardstick F ...] [--merge F] [--out F]
"""
import argparse
import ctypes
import json
import os
import signal
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CASES = [("robots_1", 1, 2, 1), ("robots_16", 16, 2, 1), ("robots_64", 64, 2, 1),
         ("grids_64_rounds_8", 64, 1, 8)]          # name, scans' owners, grids each, scans each
# configuration_files/trajectory_builder_2d.lua:100-112, free space on
OPTIONS = (0.3, 10.0, 1, 4, 0.5, 1, 0, 0.5, 0.5)


def _timed(fn, repeats, warmup):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        times.append(1e3 * (time.perf_counter() - t0))
    return dict(median=float(np.median(times)), min=float(min(times)), max=float(max(times)))


def _device_name():
    hip = ctypes.CDLL("libamdhip64.so")
    name = ctypes.create_string_buffer(256)
    if hip.hipDeviceGetName(name, 256, 0) != 0:
        return "unknown"
    return name.value.decode() or "unknown"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--library", default=None)
    ap.add_argument("--yardstick", nargs="*", default=[])
    ap.add_argument("--merge", default=None)
    ap.add_argument("--time-limit", type=int, default=300)
    ap.add_argument("--out",
                    default=os.path.join(ROOT, "profiles", "tsdf2d_insert_batch_timing.json"))
    args = ap.parse_args()
    signal.alarm(args.time_limit)
    if args.merge:
        with open(args.merge) as f:
            out = json.loads(f.read())
    else:
        out = measure(args)
    if args.yardstick:
        parents = []
        for path in args.yardstick:
            with open(path) as f:
                parents.append(json.loads(f.read()))
        for name, *_ in CASES:
            case = out["cases"][name]
            singles = [p["cases"][name]["single_calls_ms"] for p in parents]
            mean = float(np.mean(singles))
            case["parent_single_calls_ms"] = singles
            case["parent_single_calls_spread"] = (max(singles) - min(singles)) / mean
            if "batch_ms" in case:
                case["parent_single_calls_over_batch"] = mean / case["batch_ms"]
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


def measure(args):
    if args.library:
        os.environ["CMX_SO_PATH"] = os.path.abspath(args.library)
    from cartographer_amd import _lib, grid_2d, synth
    L = _lib.lib()
    has_batch = hasattr(L, "cmx_tsdf2d_insert_batch")
    _, lim, world = synth.make_submap(7, 400, 400, 0.05, 30, 1000, 10.0, 0.01)
    options = _lib.TSDFInserterOptions2D(*OPTIONS)

    def scan(k):
        at = world.free_pose(100 + k, 0.5)
        pts = world.scan(at, 1000, 10.0, 0.01, k).astype(np.float64)
        c, s = np.cos(at[2]), np.sin(at[2])
        in_map = np.zeros((pts.shape[0], 3), np.float32)
        in_map[:, 0] = at[0] + c * pts[:, 0] - s * pts[:, 1]
        in_map[:, 1] = at[1] + s * pts[:, 0] + c * pts[:, 1]
        return np.array([at[0], at[1], 0.0], np.float32), in_map

    def new_grid():
        return grid_2d.TSDF2DOnDevice(0.05, (lim["max_x"], lim["max_y"]), 400, 400, 0.3, 10.0)

    out = dict(repeats=args.repeats, warmup=args.warmup, rays=1000,
               library="this tree" if not args.library else "other build", device=_device_name(),
               hw_queues=os.environ.get("GPU_MAX_HW_QUEUES", "default"), cases={})
    for name, owners, grids_each, scans_each in CASES:
        scans = [scan(k) for k in range(owners * scans_each)]
        # insertion list: (grid index, scan index)
        plan = [(o * grids_each + g, o * scans_each + s) for o in range(owners)
                for s in range(scans_each) for g in range(grids_each)]
        num_grids = owners * grids_each
        single_grids = [new_grid() for _ in range(num_grids)]
        single_args = [(single_grids[g]._h, scans[s][0].ctypes.data, scans[s][1].ctypes.data,
                        scans[s][1].shape[0], ctypes.byref(options)) for g, s in plan]

        def singles():
            for a in single_args:
                if L.cmx_tsdf2d_insert(*a) != _lib.OK:
                    raise RuntimeError(L.cmx_last_error().decode())

        case = dict(insertions=len(plan), grids=num_grids,
                    points_min=min(s[1].shape[0] for s in scans),
                    points_max=max(s[1].shape[0] for s in scans))
        t = _timed(singles, args.repeats, args.warmup)
        case["single_calls_ms"] = t["median"]
        case["single_calls_min_max_ms"] = [t["min"], t["max"]]
        if has_batch:
            batch_grids = [new_grid() for _ in range(num_grids)]
            items = (_lib.TSDF2DInsertion * len(plan))()
            debug_items = (_lib.DebugTSDF2DInsertion * len(plan))()
            for item, debug_item, (g, s) in zip(items, debug_items, plan):
                item.grid, item.origin_xyz = batch_grids[g]._h, scans[s][0].ctypes.data
                item.returns_xyz, item.num_returns = scans[s][1].ctypes.data, scans[s][1].shape[0]
                debug_item.grid, debug_item.origin_xyz = g, item.origin_xyz
                debug_item.returns_xyz, debug_item.num_returns = item.returns_xyz, item.num_returns

            def batch():
                if L.cmx_tsdf2d_insert_batch(items, len(plan), ctypes.byref(options)) != _lib.OK:
                    raise RuntimeError(L.cmx_last_error().decode())

            limits = (_lib.Grid2DLimits * num_grids)(*[
                _lib.Grid2DLimits(0.05, lim["max_x"], lim["max_y"], 400, 400, 0.0, 0.0)
                for _ in range(num_grids)])
            rounds = np.empty(len(plan), np.int32)
            rays = np.empty(len(plan), np.int32)
            at = (_lib.Grid2DLimits * len(plan))()
            prepared = ctypes.c_int32()

            def host_plan():
                if L.cmx_debug_tsdf2d_insert_plan(limits, num_grids, debug_items, len(plan),
                                                  ctypes.byref(options), rounds.ctypes.data, at,
                                                  rays.ctypes.data,
                                                  ctypes.byref(prepared)) != _lib.OK:
                    raise RuntimeError(L.cmx_last_error().decode())

            t = _timed(batch, args.repeats, args.warmup)
            case["batch_ms"] = t["median"]
            case["batch_min_max_ms"] = [t["min"], t["max"]]
            case["single_calls_over_batch"] = case["single_calls_ms"] / case["batch_ms"]
            t = _timed(host_plan, args.repeats, args.warmup)
            case["plan_ms"] = t["median"]
            case["plan_min_max_ms"] = [t["min"], t["max"]]
            case["plan_share_of_batch"] = case["plan_ms"] / case["batch_ms"]
            case["scans_prepared"] = int(prepared.value)
            case["rounds"] = int(rounds.max()) + 1
            case["batch_equals_single_calls"] = all(
                a.limits == b.limits and np.array_equal(a.planes()[0], b.planes()[0]) and
                np.array_equal(a.planes()[1], b.planes()[1])
                for a, b in zip(batch_grids, single_grids))
        out["cases"][name] = case
        del single_grids, single_args
    return out


if __name__ == "__main__":
    main()
