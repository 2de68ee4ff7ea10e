#!/usr/bin/env python3
"""Timing of LocalTrajectoryBuilder3D::ScanMatch for a fleet: one cmx_rt3d_match_grid_batch call,
and one cmx_ceres3d_match_grids_batch call after it, against the same matches as single
cmx_rt3d_match_grid / cmx_ceres3d_match_grids calls; prints one JSON line and writes it to --out.

Legs: 1, 16 and 64 robots at the window of trajectory_builder_3d.lua (0.15 m / 1 degree).  Every
robot has a 0.10 m and a 0.45 m grid of its own, filled from four simulated sweeps of a hall, and
matches what the project's own filters leave of a fifth sweep (voxel filter 0.15 m, then the
adaptive filters of the lua file: 2 m / 150 points / 15 m for the real-time match and the
high-resolution pair, 4 m / 200 points / 60 m for the low-resolution pair); the counts are in the
JSON.  The Ceres calls start from the poses the real-time matches return, with the poses before
them as targets.  Per leg (median, min and max over --repeats after --warmup, host clock, every
call ends in a synchronise, the argument arrays are built once, outside the clock):
  rt_batch_ms, ceres_batch_ms       the one batched call
  rt_single_calls_ms, ceres_single_calls_ms   one single call per robot
and `batch_equals_single_calls`.
Route sweep: single matches of growing work (candidates x points) through the batched call with
the switch rt3d_batch_route at 1 (segmented route) and at 2 (single path), and the largest power
of two of work up to which the segmented route was not slower at every size measured.
--library PATH loads another build of the library (the parent commit's, for the yardstick of the
single-call legs on the same box); the batch legs and the sweep are left out where the entry point
is missing.  --yardstick F [F ...] takes such runs' JSON (before and after this one, same box) and
records their figures, their spread and the ratios to this run's; with --merge F nothing is
measured: F is an earlier run of this tree, to which the yardsticks are added.
--time-limit S ends the process after S seconds whatever it is doing.
Usage: python tools/rt3d_batch_timing.py [--repeats 20] [--warmup 3] [--library PATH]
                                         [--yardstick F ...] [--merge F] [--out F] [--no-sweep]
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
LEGS = [("robots_1", 1), ("robots_16", 16), ("robots_64", 64)]
LUA = (0.15, math.radians(1.0), 1e-1, 1e-1)
# (linear window m, angular window degrees, points): from the lua default to the shape of bench
# configuration C4 (65 536 points, 15^3 x 11^3 = 4.5 M candidates)
SWEEP = [(0.15, 1.0, 300), (0.2, 1.0, 1000), (0.2, 1.0, 8192), (0.3, 2.0, 8192),
         (0.5, 2.0, 16384), (0.7, 2.0, 65536)]


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--library", default=None)
    ap.add_argument("--yardstick", nargs="*", default=[])
    ap.add_argument("--merge", default=None)
    ap.add_argument("--no-sweep", action="store_true")
    ap.add_argument("--time-limit", type=int, default=420)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rt3d_batch_timing.json"))
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
        for name, _ in LEGS:
            leg = out["legs"][name]
            for what in ("rt", "ceres"):
                singles = [p["legs"][name][what + "_single_calls_ms"] for p in parents]
                mean = float(np.mean(singles))
                leg["parent_" + what + "_single_calls_ms"] = singles
                leg["parent_" + what + "_single_calls_spread"] = (max(singles) - min(singles)) / mean
                if what + "_batch_ms" in leg:
                    ratio = mean / leg[what + "_batch_ms"]
                    leg["parent_" + what + "_single_calls_over_batch"] = ratio
                    leg[what + "_gain_exceeds_spread"] = bool(
                        ratio - 1.0 > leg["parent_" + what + "_single_calls_spread"])
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


def measure(args):
    if args.library:
        os.environ["CMX_SO_PATH"] = os.path.abspath(args.library)
    from cartographer_amd import _lib, filters, grid_3d, synth
    from cartographer_amd import scan_matching_3d as sm3
    L = _lib.lib()
    has_batch = hasattr(L, "cmx_rt3d_match_grid_batch")
    world = synth.World3D(11, (30.0, 30.0, 6.0))
    out = dict(repeats=args.repeats, warmup=args.warmup, window_m_rad=list(LUA[:2]),
               library="this tree" if not args.library else "other build", device=_device_name(),
               legs={},
               launches_and_synchronisations_per_call=dict(
                   counted="from the code path, not from a trace",
                   rt_batch="per launch set (one set up to 2^25 candidates): 1 upload (a copy "
                            "kernel below 1 MB, else a copy command), 2 launches (score, collect), "
                            "1 read-back (copy kernel), 1 synchronisation; + the single path's for "
                            "every match that takes it",
                   ceres_batch="1 upload (copy kernel or command), 1 launch, 1 read-back, "
                               "1 synchronisation",
                   rt_single="per match: 2 launches for the padded brick, 7 copy or memset "
                             "commands and 1 synchronisation for the tables, then the bounds "
                             "search in rounds (a synchronisation with a read-back after each) or "
                             "2 launches, 1 read-back, 1 synchronisation and a copy per finalist",
                   ceres_single="per match: 2 uploads, 1 launch, 1 read-back, 1 synchronisation"))

    def robot(k):
        """Grids, clouds and poses of robot k."""
        grids = [grid_3d.HybridGridOnDevice(0.10), grid_3d.HybridGridOnDevice(0.45)]
        for s in range(4):
            position = world.free_position(700 + 4 * (k % 8) + s, 0.5)
            cloud = world.scan(position, 0.0, 16, 256, np.deg2rad(20.0), 40.0, 0.01, 31 * k + s)
            in_map = np.ascontiguousarray(cloud + position.astype(np.float32), np.float32)
            for g in grids:
                g.insert(position.astype(np.float32), in_map, 0.55, 0.49, 2)
        sweep = world.scan(position, 0.0, 32, 512, np.deg2rad(20.0), 40.0, 0.01, 977 + k)
        voxel = filters.voxel_filter(sweep, 0.15)
        high = np.ascontiguousarray(filters.adaptive_voxel_filter(voxel, 2.0, 150, 15.0))
        low = np.ascontiguousarray(filters.adaptive_voxel_filter(voxel, 4.0, 200, 60.0))
        offset = np.array([0.04, -0.03, 0.01]) * (1 + (k % 3))
        pose = sm3.Rigid3d(tuple(position + offset),
                           (math.cos(0.004 * (k % 5)), 0.0, 0.0, math.sin(0.004 * (k % 5))))
        return grids, high, low, pose

    rt = sm3.RealTimeCorrelativeScanMatcher3D(*LUA)
    ceres = sm3.CeresScanMatcher3D([1.0, 6.0], 5.0, 4e2, max_num_iterations=12)
    robots = [robot(k) for k in range(max(n for _, n in LEGS))]
    for name, num in LEGS:
        fleet = robots[:num]
        poses = [r[3] for r in fleet]
        high = [r[1] for r in fleet]
        hi_grids = [r[0][0] for r in fleet]
        leg = dict(robots=num, points_high=[int(len(r[1])) for r in fleet][:8],
                   points_low=[int(len(r[2])) for r in fleet][:8],
                   points_high_min_max=[int(min(len(r[1]) for r in fleet)),
                                        int(max(len(r[1]) for r in fleet))],
                   points_low_min_max=[int(min(len(r[2]) for r in fleet)),
                                       int(max(len(r[2]) for r in fleet))])
        single_results = []

        def rt_singles():
            single_results[:] = [rt.match_grid(p, c, g) for p, c, g in zip(poses, high, hi_grids)]

        t = _timed(rt_singles, args.repeats, args.warmup)
        leg["rt_single_calls_ms"], leg["rt_single_calls_min_max_ms"] = t["median"], [t["min"], t["max"]]
        matched = [p for _, p in single_results]
        targets = [np.array(p.translation) for p in poses]
        pairs = [[(r[1], r[0][0]), (r[2], r[0][1])] for r in fleet]
        refined = []

        def ceres_singles():
            refined[:] = [ceres.match_grids(t, p, e) for t, p, e in zip(targets, matched, pairs)]

        t = _timed(ceres_singles, args.repeats, args.warmup)
        leg["ceres_single_calls_ms"] = t["median"]
        leg["ceres_single_calls_min_max_ms"] = [t["min"], t["max"]]
        if has_batch:
            plan = sm3.rt3d_batch_plan(rt, [0.1] * num, [len(c) for c in high],
                                       [float(np.linalg.norm(c, axis=1).max()) for c in high])
            leg["candidates_min_max"] = [min(p["T"] * p["R"] for p in plan),
                                         max(p["T"] * p["R"] for p in plan)]
            leg["routes"] = sorted({p["route"] for p in plan})
            leg["launch_sets"] = len({p["set"] for p in plan if p["set"] >= 0})
            batch_results = []

            def rt_batch():
                batch_results[:] = rt.match_grid_batch(poses, high, hi_grids)

            t = _timed(rt_batch, args.repeats, args.warmup)
            leg["rt_batch_ms"], leg["rt_batch_min_max_ms"] = t["median"], [t["min"], t["max"]]
            leg["rt_single_calls_over_batch"] = leg["rt_single_calls_ms"] / leg["rt_batch_ms"]
            batch_refined = []

            def ceres_batch():
                batch_refined[:] = ceres.match_grids_batch(targets, matched, pairs)

            t = _timed(ceres_batch, args.repeats, args.warmup)
            leg["ceres_batch_ms"] = t["median"]
            leg["ceres_batch_min_max_ms"] = [t["min"], t["max"]]
            leg["ceres_single_calls_over_batch"] = leg["ceres_single_calls_ms"] / leg["ceres_batch_ms"]
            leg["batch_equals_single_calls"] = bool(
                all(np.float32(s) == np.float32(r[0]) and p == r[1] for s, p, r in
                    zip(batch_results[0], batch_results[1], single_results)) and
                batch_refined[0] == [p for p, _ in refined] and
                batch_refined[1] == [s for _, s in refined])
        out["legs"][name] = leg
    if has_batch and not args.no_sweep:
        out["route_sweep"] = sweep_routes(args, world, robots[0], sm3, _lib)
    return out


def sweep_routes(args, world, robot, sm3, _lib):
    """One match per size through the batched call, on either route."""
    grids, _, _, pose = robot
    position = np.array(pose.translation)
    # two sweeps of 64 rings, the returns within the 15 m of the adaptive filter, in random order:
    # a cloud of any size has the range (and so the angular step) of the whole
    big = np.concatenate([world.scan(position, 0.0, 64, 1024, np.deg2rad(20.0), 40.0, 0.01, 4242),
                          world.scan(position, 0.003, 64, 1024, np.deg2rad(20.0), 40.0, 0.01, 4243)])
    big = big[np.linalg.norm(big, axis=1) <= 15.0]
    near = big[np.random.default_rng(7).permutation(len(big))]
    sizes = []
    for linear, degrees, points in SWEEP:
        cloud = np.ascontiguousarray(near[:points], np.float32)
        m = sm3.RealTimeCorrelativeScanMatcher3D(linear, math.radians(degrees), 1e-1, 1e-1)
        (plan,) = sm3.rt3d_batch_plan(m, [0.1], [len(cloud)],
                                      [float(np.linalg.norm(cloud, axis=1).max())])
        work = plan["T"] * plan["R"] * len(cloud)
        repeats = args.repeats if work < 1e10 else max(3, args.repeats // 4)
        size = dict(linear_window=linear, angular_window_degrees=degrees, points=len(cloud),
                    L=plan["L"], A=plan["A"], candidates=plan["T"] * plan["R"], work=work,
                    log2_work=math.log2(work), repeats=repeats)
        results = {}
        for route, key in ((1, "segmented_ms"), (2, "single_path_ms")):
            _lib.debug_set(rt3d_batch_route=route)
            try:
                def call():
                    results[key] = m.match_grid_batch([pose], [cloud], [grids[0]])
                t = _timed(call, repeats, 2)
            finally:
                _lib.debug_reset()
            size[key], size[key.replace("_ms", "_min_max_ms")] = t["median"], [t["min"], t["max"]]
        a, b = results["segmented_ms"], results["single_path_ms"]
        size["routes_agree"] = bool(a[0][0] == b[0][0] and a[1][0] == b[1][0])
        size["segmented_not_slower"] = bool(size["segmented_ms"] <= size["single_path_ms"])
        sizes.append(size)
    threshold = 0
    for size in sizes:
        if not size["segmented_not_slower"]:
            break
        threshold = 1 << int(math.floor(size["log2_work"]))
    return dict(sizes=sizes, largest_power_of_two_not_slower=threshold,
                rule="the largest power of two of work not above the last size up to which the "
                     "segmented route was not slower at every size measured")


if __name__ == "__main__":
    main()
