#!/usr/bin/env python3
"""Timing of the Ceres match of LocalTrajectoryBuilder2D::ScanMatch for a fleet: one
cmx_ceres2d_match_grid_batch call against the same matches as single cmx_ceres2d_match_grid /
cmx_ceres2d_match_tsdf_grid calls; prints one JSON line and writes it to --out.

Legs: 1, 16 and 64 robots on probability grids, on TSDFs, and mixed (kinds alternating).  Every
robot has a resident 200 x 200 grid at 0.05 m of its own of either kind, filled from three
simulated scans of a 10 m room, and matches what the adaptive voxel filter of
trajectory_builder_2d.lua (0.5 m / 200 points / 50 m) leaves of a fourth scan; the counts are in
the JSON.  Ceres options of that file: weights 1 / 10 / 40, 20 iterations.  The target is the
robot's pose, the initial estimate a few centimetres from it.  Per leg (median, min and max over
--repeats after --warmup, host clock, every call ends in a synchronise):
  batch_ms            the one batched call
  single_calls_ms     one single call per robot
and `batch_equals_single_calls`.
--library PATH loads another build of the library (the parent commit's, for the yardstick of the
single-call legs on the same box); the batch legs are left out where the entry point is missing.
--yardstick F [F ...] takes such runs' JSON (before and after this one, same box) and records
their figures, their spread and the ratios to this run's; with --merge F nothing is measured: F is
an earlier run of this tree, to which the yardsticks are added.
--time-limit S ends the process after S seconds whatever it is doing.
Usage: python tools/ceres2d_batch_timing.py [--repeats 20] [--warmup 3] [--library PATH]
                                            [--yardstick F ...] [--merge F] [--out F]
"""
import argparse
import ctypes as C
import json
import math
import os
import signal
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ROBOTS = [1, 16, 64]
KINDS = ["probability", "tsdf", "mixed"]
RES, CELLS = 0.05, 200
LUA_CERES = (1.0, 10.0, 40.0, False, 20)
LUA_FILTER = (0.5, 200, 50.0)
LUA_TSDF = dict(truncation_distance=0.3, maximum_weight=10.0, update_free_space=False,
                num_normal_samples=4, sample_radius=0.5, project_sdf_distance_to_scan_normal=True,
                update_weight_range_exponent=0, angle_kernel_bandwidth=0.5,
                distance_kernel_bandwidth=0.5)


def _legs():
    return [(f"{kind}_robots_{num}", kind, num) for kind in KINDS for num in ROBOTS]


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
    hip = C.CDLL("libamdhip64.so")
    name = C.create_string_buffer(256)
    if hip.hipDeviceGetName(name, 256, 0) != 0:
        return "unknown"
    return name.value.decode() or "unknown"


def _in_map(pose, points):
    c, s = math.cos(pose[2]), math.sin(pose[2])
    out = np.array(points, np.float32, copy=True)
    out[:, 0] = pose[0] + c * points[:, 0] - s * points[:, 1]
    out[:, 1] = pose[1] + s * points[:, 0] + c * points[:, 1]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--library", default=None)
    ap.add_argument("--yardstick", nargs="*", default=[])
    ap.add_argument("--merge", default=None)
    ap.add_argument("--time-limit", type=int, default=420)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ceres2d_batch_timing.json"))
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
        for name, _, _ in _legs():
            leg = out["legs"][name]
            singles = [p["legs"][name]["single_calls_ms"] for p in parents]
            mean = float(np.mean(singles))
            leg["parent_single_calls_ms"] = singles
            leg["parent_single_calls_spread"] = (max(singles) - min(singles)) / mean
            if "batch_ms" in leg:
                ratio = mean / leg["batch_ms"]
                leg["parent_single_calls_over_batch"] = ratio
                leg["gain_exceeds_spread"] = bool(ratio - 1.0 > leg["parent_single_calls_spread"])
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


def measure(args):
    if args.library:
        os.environ["CMX_SO_PATH"] = os.path.abspath(args.library)
    from cartographer_amd import _lib, filters, grid_2d, synth
    from cartographer_amd import scan_matching as sm
    L = _lib.lib()
    has_batch = hasattr(L, "cmx_ceres2d_match_grid_batch")
    _, lim, world = synth.make_submap(7, CELLS, CELLS, RES, 12, 500, 30.0, 0.01)
    out = dict(repeats=args.repeats, warmup=args.warmup, ceres_options=list(LUA_CERES),
               library="this tree" if not args.library else "other build", device=_device_name(),
               legs={},
               launches_and_synchronisations_per_call=dict(
                   counted="from the code path, not from a trace",
                   batch="1 upload (a copy kernel below 1 MB, else a copy command), 1 launch, "
                         "1 read-back (copy kernel), 1 synchronisation",
                   single="per match: 1 upload, 1 launch, 1 read-back, 1 synchronisation"))

    def robot(k):
        """Both grids, the filtered cloud, target and initial estimate of robot k."""
        pose = world.free_pose(100 + k, 0.5)
        max_xy = (lim["max_x"], lim["max_y"])
        grid = grid_2d.ProbabilityGridOnDevice(RES, max_xy, CELLS, CELLS)
        tsdf = grid_2d.TSDF2DOnDevice(RES, max_xy, CELLS, CELLS, 0.3, 10.0)
        for s in range(3):
            at = pose + np.array([0.15 * (s - 1), 0.1 * (1 - s), 0.4 * s])
            points = _in_map(at, world.scan(at, 400, 30.0, 0.01, 31 * k + s))
            grid.insert(at[:2], points)
            tsdf.insert([at[0], at[1], 0.0], points, **LUA_TSDF)
        scan = world.scan(pose, 1000, 30.0, 0.01, 977 + k)
        cloud = np.ascontiguousarray(filters.adaptive_voxel_filter(scan, *LUA_FILTER))
        offset = np.array([0.03, -0.02, 0.01]) * (1 + (k % 3))
        initial = sm.Rigid2d(*(pose + offset))
        return grid, tsdf, cloud, np.array(pose[:2]), initial

    ceres = sm.CeresScanMatcher2D(*LUA_CERES)
    robots = [robot(k) for k in range(max(ROBOTS))]
    for name, kind, num in _legs():
        fleet = robots[:num]
        grids = [r[1] if kind == "tsdf" or (kind == "mixed" and k % 2) else r[0]
                 for k, r in enumerate(fleet)]
        clouds = [r[2] for r in fleet]
        targets = [r[3] for r in fleet]
        initials = [r[4] for r in fleet]
        counts = [int(len(c)) for c in clouds]
        limits = [g.limits for g in grids]
        leg = dict(robots=num, kind=kind, points=counts[:8], points_min_max=[min(counts), max(counts)],
                   grid_cells_min_max=[min(g["num_x_cells"] * g["num_y_cells"] for g in limits),
                                       max(g["num_x_cells"] * g["num_y_cells"] for g in limits)])
        single_results = []

        def singles():
            single_results[:] = [ceres.match(t, i, c, g)
                                 for t, i, c, g in zip(targets, initials, clouds, grids)]

        t = _timed(singles, args.repeats, args.warmup)
        leg["single_calls_ms"], leg["single_calls_min_max_ms"] = t["median"], [t["min"], t["max"]]
        leg["terminations"] = sorted({s["termination"] for _, s in single_results})
        if has_batch:
            batch_results = []

            def batch():
                batch_results[:] = ceres.match_batch(targets, initials, clouds, grids)

            t = _timed(batch, args.repeats, args.warmup)
            leg["batch_ms"], leg["batch_min_max_ms"] = t["median"], [t["min"], t["max"]]
            leg["single_calls_over_batch"] = leg["single_calls_ms"] / leg["batch_ms"]
            leg["batch_equals_single_calls"] = bool(
                batch_results[0] == [p for p, _ in single_results] and
                batch_results[1] == [s for _, s in single_results])
        out["legs"][name] = leg
    return out


if __name__ == "__main__":
    main()
