#!/usr/bin/env python3
"""Timing of FastCorrelativeScanMatcher3D creation from a resident C5-sized submap; prints one
JSON line.

The submap is tests/test_gpu_3d.py::test_fast3d_c5_sized_submap's: a 15 x 15 x 7.5 m room at
0.10 m (high) and 0.45 m (low) from eight 32 x 512 sweeps, here inserted into resident grids
(cmx_grid3d).  Options: pose_graph.lua's (depth 8, full-resolution depth 3), 120-bin histogram.
Legs (median over --repeats creations after --warmup, host clock; creation ends in a synchronise):
  from_device_grids_ms     cmx_fast3d_create_from_grids on the two grids
  download_and_create_ms   cmx_grid3d_download of both grids, then cmx_fast3d_create on the lists
Usage: python tools/fast3d_create_timing.py [--repeats 20] [--warmup 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _median_ms(fn, repeats, warmup):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        times.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    from cartographer_amd import grid_3d, synth, scan_matching_3d as sm3
    size = (15.0, 15.0, 7.5)
    world = synth.World3D(42, size)
    high, low = grid_3d.HybridGridOnDevice(0.1), grid_3d.HybridGridOnDevice(0.45)
    for p in range(8):                     # synth.make_submap_3d(42, ..., 8, 32, 512)
        pos = world.free_position(42 * 1009 + p, 0.5)
        yaw = 0.37 * p
        sensor = world.scan(pos, yaw, 32, 512, seed=42 * 31 + p).astype(np.float64)
        c, s = np.cos(yaw), np.sin(yaw)
        in_map = np.stack([pos[0] + c * sensor[:, 0] - s * sensor[:, 1],
                           pos[1] + s * sensor[:, 0] + c * sensor[:, 1],
                           pos[2] + sensor[:, 2]], 1).astype(np.float32)
        for g in (high, low):
            g.insert(pos.astype(np.float32), in_map, 0.7, 0.4, 2)
    rng = np.random.default_rng(1)
    hist = rng.uniform(0.0, 1.0, 120).astype(np.float32)
    opt = dict(branch_and_bound_depth=8, full_resolution_depth=3)

    def resident():
        sm3.FastCorrelativeScanMatcher3D.from_device_grids(high, low, hist, **opt)

    def download():
        sm3.FastCorrelativeScanMatcher3D(0.1, high.voxels(), high.grid_size, 0.45, low.voxels(),
                                         hist, **opt)

    out = dict(high_voxels=len(high.voxels()), low_voxels=len(low.voxels()),
               grid_size=high.grid_size,
               from_device_grids_ms=_median_ms(resident, args.repeats, args.warmup),
               download_and_create_ms=_median_ms(download, args.repeats, args.warmup),
               repeats=args.repeats)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
