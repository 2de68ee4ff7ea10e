#!/usr/bin/env python3
"""Timing of range data into many resident hybrid grids: one cmx_grid3d_insert_batch call against
the same insertions as single cmx_grid3d_insert calls; prints one JSON line and writes it to --out.

The clouds are 64-ring sweeps of a simulated hall (about 65 000 returns), the nearest 20 000 of
them being the "near" cloud; a robot has two submaps whose frames differ by a translation, and
every submap a 0.10 m grid for the near cloud and a 0.45 m grid for the full one: the four
insertions of ActiveSubmaps3D::InsertData.  The warm-up calls grow the bricks; afterwards no grid
grows, so every repeat does the same work.  num_free_space_voxels is 2.  Cases:
  robots_1, robots_16, robots_64   N robots x 4 insertions into 4 grids each
  grids_16_rounds_8                16 grids (0.10 m and 0.45 m alternating) x 8 clouds each, grid
                                   after grid in the list
Legs per case (median, min and max over --repeats after --warmup, host clock; every call ends in a
synchronise; the argument arrays are built once, outside the clock):
  batch_ms          one cmx_grid3d_insert_batch call for the whole list
  single_calls_ms   one cmx_grid3d_insert call per insertion, in list order, into grids of their own
and `batch_equals_single_calls`: grid_size and every voxel of every grid afterwards.
--library PATH loads another build of the library (the parent commit's, for the yardstick of
single_calls_ms on the same box); the batch leg is left out where the entry point is missing.
--yardstick F [F ...] takes such runs' JSON (before and after this one, same box) and records
their figures, their spread and the ratios to this run's; with --merge F nothing is measured: F
is an earlier run of this tree, to which the yardsticks are added.
--dropin NEW PARENT runs two builds of the resident LocalTrajectoryBuilder3D drive (this tree's and
the parent commit's) alternately, three times each, and records the per-AddRangeData medians they
print; --parent-library-dir DIR is put in front of the parent build's library search path.
--time-limit S ends the process after S seconds whatever it is doing.
Writes profiles/grid3d_insert_batch_timing.json unless --out names another file.
Usage: python tools/grid3d_insert_batch_timing.py [--repeats 20] [--warmup 3] [--library PATH]
                                                  [--yardstick F ...] [--merge F] [--out F]
                                                  [--dropin NEW PARENT] [--parent-library-dir DIR]
"""
import argparse
import ctypes
import json
import os
import re
import signal
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CASES = [("robots_1", 1), ("robots_16", 16), ("robots_64", 64), ("grids_16_rounds_8", 0)]
NEAR, FREE, HIT, MISS = 20000, 2, 0.55, 0.49


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
    ap.add_argument("--dropin", nargs=2, default=None, metavar=("NEW", "PARENT"))
    ap.add_argument("--parent-library-dir", default=None)
    ap.add_argument("--time-limit", type=int, default=420)
    ap.add_argument("--out",
                    default=os.path.join(ROOT, "profiles", "grid3d_insert_batch_timing.json"))
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
        for name, _ in CASES:
            case = out["cases"][name]
            singles = [p["cases"][name]["single_calls_ms"] for p in parents]
            mean = float(np.mean(singles))
            case["parent_single_calls_ms"] = singles
            case["parent_single_calls_spread"] = (max(singles) - min(singles)) / mean
            if "batch_ms" in case:
                case["parent_single_calls_over_batch"] = mean / case["batch_ms"]
    if args.dropin:
        out["dropin_local_trajectory_builder_3d"] = dropin(args)
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


def dropin(args):
    """The two builds alternately, three runs each: the median per AddRangeData each run prints."""
    builds = dict(new=(args.dropin[0], None), parent=(args.dropin[1], args.parent_library_dir))
    medians, outputs = dict(new=[], parent=[]), dict(new=[], parent=[])
    for _ in range(3):
        for key in ("parent", "new"):
            path, library_dir = builds[key]
            env = dict(os.environ)
            if library_dir:
                env["LD_LIBRARY_PATH"] = os.pathsep.join(
                    [os.path.abspath(library_dir)] + [p for p in [env.get("LD_LIBRARY_PATH")] if p])
            run = subprocess.run([path], capture_output=True, text=True, timeout=300, env=env)
            if run.returncode != 0:
                raise RuntimeError(f"{path} ended with {run.returncode}: {run.stderr[-400:]}")
            m = re.search(r"median ([0-9.]+) ms", run.stderr)
            medians[key].append(float(m.group(1)))
            outputs[key].append(run.stdout)
    spread = (max(medians["parent"]) - min(medians["parent"])) / float(np.mean(medians["parent"]))
    return dict(new_median_ms=medians["new"], parent_median_ms=medians["parent"],
                parent_spread=spread,
                parent_over_new=float(np.median(medians["parent"]) / np.median(medians["new"])),
                outputs_identical=len(set(outputs["new"] + outputs["parent"])) == 1)


def measure(args):
    if args.library:
        os.environ["CMX_SO_PATH"] = os.path.abspath(args.library)
    from cartographer_amd import _lib, grid_3d, synth
    L = _lib.lib()
    has_batch = hasattr(L, "cmx_grid3d_insert_batch")
    world = synth.World3D(11, (30.0, 30.0, 6.0))

    def sweep(k):
        position = world.free_position(300 + k, 0.5)
        cloud = world.scan(position, 0.21 * k, 64, 1024, np.deg2rad(20.0), 40.0, 0.01, k)
        near = cloud[np.argsort(np.linalg.norm(cloud, axis=1), kind="stable")[:NEAR]]
        return np.ascontiguousarray(cloud, np.float32), np.ascontiguousarray(near, np.float32)

    sweeps = [sweep(k) for k in range(8)]
    frames = [np.array([1.5, -2.0, 0.3], np.float32), np.array([-4.0, 3.0, -0.2], np.float32)]

    def robot(k):
        """(resolution, origin, cloud) of the four insertions of robot k's step."""
        cloud, near = sweeps[k % len(sweeps)]
        out = []
        for frame in frames:
            origin = frame + np.float32(0.01 * k)
            out.append((0.10, origin, near + origin))
            out.append((0.45, origin, cloud + origin))
        return out

    out = dict(repeats=args.repeats, warmup=args.warmup, num_free_space_voxels=FREE,
               library="this tree" if not args.library else "other build", device=_device_name(),
               cases={})
    for name, robots in CASES:
        # insertion list: (grid index, origin, cloud); resolutions by grid
        plan, resolutions = [], []
        if robots:
            for k in range(robots):
                for resolution, origin, cloud in robot(k):
                    plan.append((len(resolutions), origin, cloud))
                    resolutions.append(resolution)
        else:
            for g in range(16):
                resolutions.append(0.10 if g % 2 == 0 else 0.45)
                for r in range(8):
                    resolution, origin, cloud = robot(g + 16 * r)[g % 2]
                    plan.append((g, origin, cloud))
        single_grids = [grid_3d.HybridGridOnDevice(r) for r in resolutions]
        single_args = [(single_grids[g]._h, o.ctypes.data, c.ctypes.data, c.shape[0], HIT, MISS,
                        FREE) for g, o, c in plan]

        def singles():
            for a in single_args:
                if L.cmx_grid3d_insert(*a) != _lib.OK:
                    raise RuntimeError(L.cmx_last_error().decode())

        case = dict(insertions=len(plan), grids=len(resolutions),
                    returns_min=min(c.shape[0] for _, _, c in plan),
                    returns_max=max(c.shape[0] for _, _, c in plan))
        t = _timed(singles, args.repeats, args.warmup)
        case["single_calls_ms"] = t["median"]
        case["single_calls_min_max_ms"] = [t["min"], t["max"]]
        if has_batch:
            batch_grids = [grid_3d.HybridGridOnDevice(r) for r in resolutions]
            items = (_lib.Grid3DInsertion * len(plan))()
            for item, (g, o, c) in zip(items, plan):
                item.grid, item.origin_xyz = batch_grids[g]._h, o.ctypes.data
                item.returns_xyz, item.num_returns = c.ctypes.data, c.shape[0]

            def batch():
                if L.cmx_grid3d_insert_batch(items, len(plan), HIT, MISS, FREE) != _lib.OK:
                    raise RuntimeError(L.cmx_last_error().decode())

            t = _timed(batch, args.repeats, args.warmup)
            case["batch_ms"] = t["median"]
            case["batch_min_max_ms"] = [t["min"], t["max"]]
            case["single_calls_over_batch"] = case["single_calls_ms"] / case["batch_ms"]
            case["batch_equals_single_calls"] = all(
                a.grid_size == b.grid_size and np.array_equal(a.voxels(), b.voxels())
                for a, b in zip(batch_grids, single_grids))
            case["known_voxels_max"] = max(len(g.voxels()) for g in batch_grids[:4])
            del batch_grids, items
        out["cases"][name] = case
        del single_grids, single_args
    return out


if __name__ == "__main__":
    main()
