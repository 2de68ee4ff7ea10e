#!/usr/bin/env python3
"""Timing of many nodes against one 2D submap in one call (cmx_fast2d_match_pairs /
cmx_fast2d_refine_pairs: the burst of PoseGraph2D::ComputeConstraintsForNode when a submap
finishes) and of cmx_fast2d_create_from_grid; prints one JSON line and writes it to --out.

The submap is the benchmark's: a 400 x 400 grid at 0.05 m from 30 scans, resident in HBM
(ProbabilityGridOnDevice); the matcher is built from it in place with pose_graph.lua's options
(depth 7, windows 7 m / 30 deg).  32 distinct nodes, a scan each from its own free pose, of 200
and 1000 beams in turn, windowed searches around a displaced pose against min_score 0.55.
Legs (median, min and max over --repeats after --warmup, host clock; every call ends in a
synchronise):
  match_pairs_ms         one cmx_fast2d_match_pairs call for the 32 (node, submap) pairs
  single_calls_ms        32 cmx_fast2d_match calls, one per node
  refine_pairs_ms        one cmx_fast2d_refine_pairs call for the 32 results
  refine_batch_calls_ms  32 cmx_fast2d_refine_batch calls of one pair
  create_from_grid_ms    cmx_fast2d_create_from_grid of the submap (and the destroy)
gpu_max_hw_queues is GPU_MAX_HW_QUEUES as the process sees it once the library is loaded (the
library's default of 16 does not override a set value): the gain of concurrent groups depends
on it.
--library PATH loads another build of the library (the parent commit's, for the yardstick of
single_calls_ms and create_from_grid_ms on the same box); legs whose entry point it lacks are
left out.  --yardstick F [F ...] takes such runs' JSON (before and after this one, same box)
and records their figures, their spread and the ratios to this run's; with --merge F nothing is
measured: F is an earlier run of this tree, to which the yardsticks are added.
Writes profiles/fast2d_pairs_timing.json unless --out names another file.
Usage: python tools/fast2d_pairs_timing.py [--repeats 20] [--warmup 3] [--library PATH]
                                           [--yardstick F ...] [--merge F] [--out F]
"""
import argparse
import ctypes
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NODES = 32


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


def _getenv(name):
    getenv = ctypes.CDLL(None).getenv
    getenv.restype = ctypes.c_char_p
    value = getenv(name.encode())
    return None if value is None else value.decode()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--library", default=None)
    ap.add_argument("--yardstick", nargs="*", default=[])
    ap.add_argument("--merge", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fast2d_pairs_timing.json"))
    args = ap.parse_args()
    if args.merge:
        with open(args.merge) as f:
            out = json.loads(f.read())
    else:
        out = measure(args)
    if args.yardstick and "match_pairs_ms" in out:
        parents = []
        for path in args.yardstick:
            with open(path) as f:
                parents.append(json.loads(f.read()))
        out["parent_single_calls_ms"] = [p["single_calls_ms"] for p in parents]
        out["parent_create_from_grid_ms"] = [p["create_from_grid_ms"] for p in parents]
        mean = float(np.mean(out["parent_single_calls_ms"]))
        out["parent_single_calls_spread"] = \
            (max(out["parent_single_calls_ms"]) - min(out["parent_single_calls_ms"])) / mean
        out["parent_single_calls_over_match_pairs"] = mean / out["match_pairs_ms"]
        out["parent_create_over_create"] = \
            float(np.mean(out["parent_create_from_grid_ms"])) / out["create_from_grid_ms"]
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


def measure(args):
    if args.library:
        os.environ["CMX_SO_PATH"] = os.path.abspath(args.library)
    from cartographer_amd import _lib, grid_2d, synth, scan_matching as sm
    L = _lib.lib()
    cells, lim, world = synth.make_submap(7, 400, 400, 0.05, 30, 1000, 10.0, 0.01)
    grid = grid_2d.ProbabilityGridOnDevice(0.05, (lim["max_x"], lim["max_y"]), 400, 400, cells)
    depth, lin, ang = 7, 7.0, math.radians(30.0)
    matcher = grid.fast_matcher(depth, lin, ang)
    rng = np.random.default_rng(1)
    clouds, initial = [], []
    for k in range(NODES):
        truth = world.free_pose(100 + k, 0.5)
        clouds.append(world.scan(truth, 1000 if k % 2 else 200, 10.0, 0.01, k))
        d = rng.uniform(-0.8, 0.8, 2)
        initial.append(sm.Rigid2d(float(truth[0] + d[0]), float(truth[1] + d[1]),
                                  float(truth[2] + rng.uniform(-0.1, 0.1))))
    min_score = 0.55
    matchers = [matcher] * NODES

    def singles():
        return [matcher.match(pose, cloud, min_score) for pose, cloud in zip(initial, clouds)]

    def pairs():
        return sm.match_pairs(matchers, initial, [0] * NODES, [min_score] * NODES, clouds)

    def create():
        grid.fast_matcher(depth, lin, ang).__del__()

    expected = singles()
    points = sorted(len(c) for c in clouds)
    out = dict(nodes=NODES, points_min=points[0], points_max=points[-1],
               found=sum(bool(r[0]) for r in expected), repeats=args.repeats,
               library="this tree" if not args.library else "other build", device=_device_name(),
               gpu_max_hw_queues=_getenv("GPU_MAX_HW_QUEUES"))

    def leg(name, fn):
        t = _timed(fn, args.repeats, args.warmup)
        out[name] = t["median"]
        out[name.replace("_ms", "_min_max_ms")] = [t["min"], t["max"]]

    leg("single_calls_ms", singles)
    leg("create_from_grid_ms", create)
    if hasattr(L, "cmx_fast2d_match_pairs"):
        found, scores, poses, _ = pairs()
        out["pairs_equal_single_calls"] = all(
            bool(found[k]) == bool(e[0]) and (not e[0] or (
                np.float32(scores[k]) == np.float32(e[1]) and
                (poses[k].x, poses[k].y, poses[k].theta) == (e[2].x, e[2].y, e[2].theta)))
            for k, e in enumerate(expected))
        leg("match_pairs_ms", pairs)
        out["single_calls_over_match_pairs"] = out["single_calls_ms"] / out["match_pairs_ms"]
        ceres = sm.CeresScanMatcher2D(20.0, 10.0, 1.0, True, 10)

        def refine_pairs():
            return ceres.refine_pairs(matchers, found, poses, clouds)

        def refine_calls():
            return [ceres.refine_batch([matcher], [int(found[k])], [poses[k]], clouds[k])
                    for k in range(NODES)]

        one_call, by_calls = refine_pairs(), refine_calls()
        out["refine_pairs_equal_refine_batch_calls"] = all(
            one_call[0][k] == by_calls[k][0][0] and one_call[1][k] == by_calls[k][1][0]
            for k in range(NODES))
        leg("refine_pairs_ms", refine_pairs)
        leg("refine_batch_calls_ms", refine_calls)
        out["refine_batch_calls_over_refine_pairs"] = \
            out["refine_batch_calls_ms"] / out["refine_pairs_ms"]
    return out


if __name__ == "__main__":
    main()
