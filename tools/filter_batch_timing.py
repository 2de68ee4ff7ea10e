#!/usr/bin/env python3
"""Timing of the local trajectory builders' filter chains for a fleet in one cmx_filter_batch call
against one single call per filter; prints one JSON line and writes it to --out.

Two chains, for N in --robots (default 1, 16, 64) robots with a cloud each (distinct seeds):
  2d   a 1000-point planar scan: VoxelFilter 0.025, then AdaptiveVoxelFilter 0.5 / 200 / 50 on its
       output (trajectory_builder_2d.lua)
  3d   a 4000-point cloud: VoxelFilter 0.15, then AdaptiveVoxelFilter 2.0 / 150 / 15 and
       4.0 / 200 / 60 on its output (trajectory_builder_3d.lua)
Every filter returns its points (no indices).  Legs, per chain and N (host clock around the whole
fleet's filters, every call ends in a synchronise; median, min and max over --repeats after
--warmup):
  batch_ms     one cmx_filter_batch call, the chained filters reading their parents' output on the
               device
  singles_ms   cmx_voxel_filter per robot, then cmx_adaptive_voxel_filter on the points it
               returned: 2 N or 3 N calls, the intermediate clouds through the host
Before anything is timed the batch's counts and points are compared with the single calls'
("results_equal").  Of the batch call the debug switch host_trace reports, per call (medians over
five calls, microseconds of the host's clock): prepare (plan, descriptors, clouds into the pinned
block), issue (the upload and the launches), wait (the synchronisation), copy (results out of the
pinned block); "prepare_share" is prepare / the four together.
--library PATH loads another build of the library (the parent commit's, for the yardstick on the
same box): only the singles legs are measured.  --yardstick F [F ...] takes such runs' JSON (before
and after this one) and records their figures, their spread and the ratio to this run's batch leg;
"batch_beats_parent" only where the batch is below the parent's fastest run by more than the
parent's own spread.  With --merge F nothing is measured: F is an earlier run of this tree.
Writes profiles/filter_batch_timing.json unless --out names another file.
Usage: python tools/filter_batch_timing.py [--robots 1 16 64] [--repeats 20] [--warmup 3]
                                           [--library PATH] [--yardstick F ...] [--merge F]
                                           [--out F]
"""
import argparse
import ctypes as C
import json
import os
import re
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
# (mode, length, min_num_points, max_range, parent within the chain)
CHAINS = {
    "2d": dict(points=1000, filters=[(0, 0.025, 0.0, 0.0, -1), (1, 0.5, 200.0, 50.0, 0)]),
    "3d": dict(points=4000, filters=[(0, 0.15, 0.0, 0.0, -1), (1, 2.0, 150.0, 15.0, 0),
                                     (1, 4.0, 200.0, 60.0, 0)]),
}


def _cloud(chain, seed):
    rng = np.random.default_rng(seed)
    n = CHAINS[chain]["points"]
    if chain == "2d":
        angle = np.sort(rng.uniform(-np.pi, np.pi, n))
        r = 8.0 + 6.0 * np.sin(3.0 * angle) + rng.normal(0.0, 0.02, n)
        return np.stack([r * np.cos(angle), r * np.sin(angle), np.zeros(n)], 1).astype(np.float32)
    return (rng.normal(0.0, 8.0, (n, 3)) * np.array([1.0, 1.0, 0.2])).astype(np.float32)


def _timed(fn, repeats, warmup):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ms.append(1e3 * (time.perf_counter() - t0))
    return dict(median=float(np.median(ms)), min=float(min(ms)), max=float(max(ms)))


def _device_name():
    hip = C.CDLL("libamdhip64.so")
    name = C.create_string_buffer(256)
    if hip.hipDeviceGetName(name, 256, 0) != 0:
        return "unknown"
    return name.value.decode() or "unknown"


def _captured_stderr(fn):
    """fn() with the process's stderr (the library writes there) going to a file; its text."""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile() as f:
        os.dup2(f.fileno(), 2)
        try:
            fn()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        f.seek(0)
        return f.read().decode(errors="replace")


class Fleet:
    """The clouds, output buffers and job list of `robots` robots running one chain."""

    def __init__(self, _lib, chain, robots):
        self.lib, self.L = _lib, _lib.lib()
        self.filters = CHAINS[chain]["filters"]
        self.n = CHAINS[chain]["points"]
        self.robots = robots
        self.clouds = [_cloud(chain, 1000 + r) for r in range(robots)]
        per = len(self.filters)
        self.out = [np.empty((self.n, 3), np.float32) for _ in range(robots * per)]
        self.single_out = [np.empty((self.n, 3), np.float32) for _ in range(robots * per)]
        self.kept = np.zeros(robots * per, np.int32)
        self.single_kept = np.zeros(robots * per, np.int32)
        self.jobs = None
        if hasattr(self.L, "cmx_filter_batch"):
            # all roots first, then the chained jobs (any order with parents first would do)
            self.order = [(r, f) for f in range(per) for r in range(robots)]
            self.jobs = (_lib.FilterJob * len(self.order))()
            index = {rf: k for k, rf in enumerate(self.order)}
            for k, (r, f) in enumerate(self.order):
                mode, length, min_points, max_range, parent = self.filters[f]
                job = self.jobs[k]
                job.mode, job.length = mode, length
                job.min_num_points, job.max_range = min_points, max_range
                job.input_job = -1 if parent < 0 else index[(r, parent)]
                if parent < 0:
                    job.point_cloud_xyz = self.clouds[r].ctypes.data
                    job.num_points = self.n
                job.filtered_xyz = self.out[r * per + f].ctypes.data

    def batch(self):
        kept = np.zeros(len(self.order), np.int32)
        self.lib.check(self.L.cmx_filter_batch(self.jobs, len(self.order), 0, kept.ctypes.data))
        per = len(self.filters)
        for k, (r, f) in enumerate(self.order):
            self.kept[r * per + f] = kept[k]

    def singles(self):
        L, check, per = self.L, self.lib.check, len(self.filters)
        kept = C.c_int32()
        for r in range(self.robots):
            for f, (mode, length, min_points, max_range, parent) in enumerate(self.filters):
                out = self.single_out[r * per + f]
                if parent < 0:
                    src, n = self.clouds[r], self.n
                else:
                    src, n = self.single_out[r * per + parent], int(self.single_kept[r * per + parent])
                if mode == 0:
                    check(L.cmx_voxel_filter(src.ctypes.data, n, length, 0, out.ctypes.data,
                                             C.byref(kept)))
                else:
                    check(L.cmx_adaptive_voxel_filter(src.ctypes.data, n, length, min_points,
                                                      max_range, 0, out.ctypes.data,
                                                      C.byref(kept)))
                self.single_kept[r * per + f] = kept.value

    def equal(self):
        self.batch()
        self.singles()
        return bool(np.array_equal(self.kept, self.single_kept) and all(
            np.array_equal(a[:n], b[:n]) for a, b, n in zip(self.out, self.single_out, self.kept)))


def measure(args):
    if args.library:
        os.environ["CMX_SO_PATH"] = os.path.abspath(args.library)
    from cartographer_amd import _lib
    L = _lib.lib()
    has_batch = hasattr(L, "cmx_filter_batch")
    out = dict(robots=list(args.robots), repeats=args.repeats, warmup=args.warmup,
               library="this tree" if not args.library else "other build",
               device=_device_name(), chains={})
    for chain in CHAINS:
        rows = {}
        for robots in args.robots:
            fleet = Fleet(_lib, chain, robots)
            row = dict(jobs=robots * len(fleet.filters))
            if has_batch:
                row["results_equal"] = fleet.equal()
                if not row["results_equal"]:
                    raise SystemExit("the batch's results differ from the single calls': nothing timed")
            t = _timed(fleet.singles, args.repeats, args.warmup)
            row["singles_ms"], row["singles_min_max_ms"] = t["median"], [t["min"], t["max"]]
            row["kept"] = [int(k) for k in fleet.single_kept[:len(fleet.filters)]]
            if has_batch:
                t = _timed(fleet.batch, args.repeats, args.warmup)
                row["batch_ms"], row["batch_min_max_ms"] = t["median"], [t["min"], t["max"]]
                row["singles_over_batch"] = row["singles_ms"] / row["batch_ms"]
                _lib.debug_set(host_trace=1)
                try:
                    text = _captured_stderr(lambda: [fleet.batch() for _ in range(5)])
                finally:
                    _lib.debug_reset()
                found = re.findall(r"filter_batch jobs=(\d+) sets=(\d+) launches=(\d+) single=(\d+) "
                                   r"prepare=(\d+) issue=(\d+) wait=(\d+) copy=(\d+)", text)
                if found:
                    cols = np.array(found, np.float64)
                    parts = {name: float(np.median(cols[:, 4 + i]))
                             for i, name in enumerate(("prepare_us", "issue_us", "wait_us",
                                                       "copy_us"))}
                    row["batch_trace"] = dict(sets=int(cols[0, 1]), launches=int(cols[0, 2]),
                                              **parts)
                    row["prepare_share"] = parts["prepare_us"] / max(sum(parts.values()), 1.0)
            rows[str(robots)] = row
        out["chains"][chain] = rows
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", type=int, nargs="*", default=[1, 16, 64])
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--library", default=None)
    ap.add_argument("--yardstick", nargs="*", default=[])
    ap.add_argument("--merge", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "filter_batch_timing.json"))
    args = ap.parse_args()
    if args.merge:
        with open(args.merge) as f:
            out = json.loads(f.read())
    else:
        out = measure(args)
    if args.yardstick and out.get("library") == "this tree":
        parents = []
        for path in args.yardstick:
            with open(path) as f:
                parents.append(json.loads(f.read()))
        for chain, rows in out["chains"].items():
            for robots, row in rows.items():
                runs = [p["chains"][chain][robots]["singles_ms"] for p in parents
                        if robots in p["chains"].get(chain, {})]
                if not runs:
                    continue
                mean = float(np.mean(runs))
                row["parent_singles_ms"] = runs
                row["parent_singles_spread"] = (max(runs) - min(runs)) / mean
                row["parent_singles_over_batch"] = mean / row["batch_ms"]
                # the batch wins where it is below the parent by more than the parent's own spread
                row["batch_beats_parent"] = bool(min(runs) - row["batch_ms"] > max(runs) - min(runs))
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
