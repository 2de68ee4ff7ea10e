#!/usr/bin/env python3
"""Timing of many nodes against one submap in one fast-3D batch (cmx_fast3d_match_pairs: the
burst of PoseGraph3D::ComputeConstraintsForNode when a submap finishes); prints one JSON line and
writes it to --out.

The submap is tests/test_gpu_3d.py::test_fast3d_c5_sized_submap's: a 15 x 15 x 7.5 m room at
0.10 m (high) and 0.45 m (low) from eight 32 x 512 sweeps, resident in HBM.  Options:
pose_graph.lua's (depth 8, full-resolution depth 3, windows 5 m / 1 m / 15 deg), 120-bin
histograms.  32 distinct nodes: a 32 x 512 sweep each from its own position and yaw, every 6th
point high-resolution, every 80th low-resolution, windowed searches around a displaced pose.
Legs (median over --repeats after --warmup, host clock; every call ends in a synchronise):
  single_calls_ms   32 cmx_fast3d_match calls, one per node
  match_pairs_ms    one cmx_fast3d_match_pairs call for the 32 (node, submap) pairs
  match_batch_ms    cmx_fast3d_match_batch of node 0 against 32 copies of the submap, for scale
--library PATH loads another build of the library (the parent commit's, for the yardstick of
single_calls_ms on the same box); legs whose entry point it lacks are left out.  --yardstick F
takes such a run's JSON and records its single_calls_ms and the ratio to match_pairs_ms.
Writes profiles/fast3d_nodes_timing.json unless --out names another file.
Usage: python tools/fast3d_nodes_timing.py [--repeats 20] [--warmup 3] [--library PATH]
                                           [--yardstick F] [--out F]
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NODES = 32


def _median_ms(fn, repeats, warmup):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        times.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(times))


def _device_name():
    import ctypes
    hip = ctypes.CDLL("libamdhip64.so")
    name = ctypes.create_string_buffer(256)
    if hip.hipDeviceGetName(name, 256, 0) != 0:
        return "unknown"
    return name.value.decode()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--library", default=None)
    ap.add_argument("--yardstick", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fast3d_nodes_timing.json"))
    args = ap.parse_args()
    if args.library:
        os.environ["CMX_SO_PATH"] = os.path.abspath(args.library)
    from cartographer_amd import _lib, synth, scan_matching_3d as sm3
    size = (15.0, 15.0, 7.5)
    grid, world = synth.make_submap_3d(42, 0.1, size, 8, 32, 512)
    low, _ = synth.make_submap_3d(42, 0.45, size, 8, 32, 512)
    rng = np.random.default_rng(1)
    hist = rng.uniform(0.0, 1.0, 120).astype(np.float32)
    hist[10:14] += 6.0
    opt = dict(branch_and_bound_depth=8, full_resolution_depth=3, min_rotational_score=0.77,
               min_low_resolution_score=0.35, linear_xy_search_window=5.0,
               linear_z_search_window=1.0, angular_search_window=math.radians(15.0))
    matcher = sm3.FastCorrelativeScanMatcher3D(0.1, grid.voxels(), grid.grid_size, 0.45,
                                               low.voxels(), hist, **opt)
    datas, poses = [], []
    for k in range(NODES):
        pos = world.free_position(77 + k, 0.6)
        yaw = 0.4 + 0.05 * k
        full = world.scan(pos, yaw, 32, 512, seed=1 + k)
        datas.append(sm3.TrajectoryNodeData(full[::6].copy(), full[::80].copy(),
                                            np.roll(hist, -19 - k % 3).copy()))
        d = rng.uniform(-0.8, 0.8, 3) * np.array([1.0, 1.0, 0.25])
        half = 0.5 * (yaw + rng.uniform(-0.1, 0.1))
        poses.append(sm3.Rigid3d(tuple(pos + d), (math.cos(half), 0.0, 0.0, math.sin(half))))
    ident = sm3.Rigid3d()
    min_score = 0.2

    def singles():
        return [matcher.match(pose, ident, data, min_score) for pose, data in zip(poses, datas)]

    def pairs():
        return sm3.fast3d_match_pairs([matcher] * NODES, poses, [ident] * NODES, [False] * NODES,
                                      [min_score] * NODES, datas)[0]

    def batch():
        return sm3.fast3d_match_batch([matcher] * NODES, [poses[0]] * NODES, [ident] * NODES,
                                      [False] * NODES, [min_score] * NODES, datas[0])[0]

    expected = singles()
    out = dict(nodes=NODES, high_points=int(datas[0].high_resolution_point_cloud.shape[0]),
               found=sum(r is not None for r in expected), repeats=args.repeats,
               library="this tree" if not args.library else "other build", device=_device_name(),
               single_calls_ms=_median_ms(singles, args.repeats, args.warmup))
    if hasattr(_lib.lib(), "cmx_fast3d_match_pairs"):
        got = pairs()
        out["pairs_equal_single_calls"] = all(
            (e is None) == (g is None) and (e is None or (
                np.float32(e["score"]) == np.float32(g["score"]) and
                e["pose_estimate"] == g["pose_estimate"])) for e, g in zip(expected, got))
        out["match_pairs_ms"] = _median_ms(pairs, args.repeats, args.warmup)
        out["single_calls_over_match_pairs"] = out["single_calls_ms"] / out["match_pairs_ms"]
    out["match_batch_ms"] = _median_ms(batch, args.repeats, args.warmup)
    if args.yardstick and "match_pairs_ms" in out:
        with open(args.yardstick) as f:
            out["parent_single_calls_ms"] = json.loads(f.read())["single_calls_ms"]
        out["parent_single_calls_over_match_pairs"] = \
            out["parent_single_calls_ms"] / out["match_pairs_ms"]
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
