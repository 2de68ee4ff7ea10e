#!/usr/bin/env python3
"""Timing of RotationalScanMatcher::ComputeHistogram for a fleet in one
cmx_compute_histogram_batch call against one cmx_compute_histogram call per robot; prints one JSON
line and writes it to --out.

Two cloud sizes, for N in --robots (default 1, 16, 64) robots with a cloud each (distinct seeds),
120 bins:
  3d   a 4000-point cloud (what the 3D builder's voxel filter keeps of a scan)
  2d   a 700-point cloud (the 2D-sized case)
Legs, per size and N (host clock around the whole fleet's histograms, every call ends in a
synchronise; median, min and max over --repeats after --warmup):
  batch_ms     one cmx_compute_histogram_batch call
  singles_ms   cmx_compute_histogram per robot: N calls
Before anything is timed the batch's histograms are compared with the single calls'
("results_equal").  Of the batch call the debug switch host_trace reports, per call (medians over
five calls, microseconds of the host's clock): prepare (the scan for non-finite coordinates, plan,
descriptors, clouds into the pinned block), issue (the upload and the launches), wait (the
synchronisation), copy (histograms out of the pinned block).
--library PATH loads another build of the library (the parent commit's, for the yardstick on the
same box): only the singles legs are measured.  --yardstick F [F ...] takes such runs' JSON (before
and after this one) and records their figures, their spread and the ratio to this run's batch leg;
"batch_beats_parent" only where the batch is below the parent's fastest run by more than the
parent's own spread.  With --merge F nothing is measured: F is an earlier run of this tree.
Writes profiles/histogram_batch_timing.json unless --out names another file.
Usage: python tools/histogram_batch_timing.py [--robots 1 16 64] [--repeats 20] [--warmup 3]
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
SIZES = {"3d": 4000, "2d": 700}
BINS = 120


def _cloud(n, seed):
    rng = np.random.default_rng(seed)
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
    """The clouds, output buffers and job list of `robots` robots with `points` points each."""

    def __init__(self, _lib, points, robots):
        self.lib, self.L = _lib, _lib.lib()
        self.n, self.robots = points, robots
        self.clouds = [_cloud(points, 1000 + r) for r in range(robots)]
        self.out = [np.zeros(BINS, np.float32) for _ in range(robots)]
        self.single_out = [np.zeros(BINS, np.float32) for _ in range(robots)]
        self.jobs = None
        if hasattr(self.L, "cmx_compute_histogram_batch"):
            self.jobs = (_lib.HistogramJob * robots)()
            for r, job in enumerate(self.jobs):
                job.point_cloud_xyz, job.num_points = self.clouds[r].ctypes.data, points
                job.histogram_size, job.histogram = BINS, self.out[r].ctypes.data

    def batch(self):
        self.lib.check(self.L.cmx_compute_histogram_batch(self.jobs, self.robots, 0))

    def singles(self):
        for cloud, out in zip(self.clouds, self.single_out):
            self.lib.check(self.L.cmx_compute_histogram(cloud.ctypes.data, self.n, BINS, 0,
                                                        out.ctypes.data))

    def equal(self):
        self.batch()
        self.singles()
        return bool(all(np.array_equal(a, b) for a, b in zip(self.out, self.single_out)))


def measure(args):
    if args.library:
        os.environ["CMX_SO_PATH"] = os.path.abspath(args.library)
    from cartographer_amd import _lib
    L = _lib.lib()
    has_batch = hasattr(L, "cmx_compute_histogram_batch")
    out = dict(robots=list(args.robots), repeats=args.repeats, warmup=args.warmup, bins=BINS,
               library="this tree" if not args.library else "other build",
               device=_device_name(), sizes={})
    for size, points in SIZES.items():
        rows = {}
        for robots in args.robots:
            fleet = Fleet(_lib, points, robots)
            row = dict(points=points)
            if has_batch:
                row["results_equal"] = fleet.equal()
                if not row["results_equal"]:
                    raise SystemExit("the batch's results differ from the single calls': nothing timed")
            t = _timed(fleet.singles, args.repeats, args.warmup)
            row["singles_ms"], row["singles_min_max_ms"] = t["median"], [t["min"], t["max"]]
            row["histogram_sum"] = float(fleet.single_out[0].sum())
            if has_batch:
                t = _timed(fleet.batch, args.repeats, args.warmup)
                row["batch_ms"], row["batch_min_max_ms"] = t["median"], [t["min"], t["max"]]
                row["singles_over_batch"] = row["singles_ms"] / row["batch_ms"]
                _lib.debug_set(host_trace=1)
                try:
                    text = _captured_stderr(lambda: [fleet.batch() for _ in range(5)])
                finally:
                    _lib.debug_reset()
                found = re.findall(r"histogram_batch jobs=(\d+) sets=(\d+) launches=(\d+) "
                                   r"single=(\d+) prepare=(\d+) issue=(\d+) wait=(\d+) copy=(\d+)",
                                   text)
                if found:
                    cols = np.array(found, np.float64)
                    parts = {name: float(np.median(cols[:, 4 + i]))
                             for i, name in enumerate(("prepare_us", "issue_us", "wait_us",
                                                       "copy_us"))}
                    row["batch_trace"] = dict(sets=int(cols[0, 1]), launches=int(cols[0, 2]),
                                              single=int(cols[0, 3]), **parts)
            rows[str(robots)] = row
        out["sizes"][size] = rows
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", type=int, nargs="*", default=[1, 16, 64])
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--library", default=None)
    ap.add_argument("--yardstick", nargs="*", default=[])
    ap.add_argument("--merge", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "histogram_batch_timing.json"))
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
        for size, rows in out["sizes"].items():
            for robots, row in rows.items():
                runs = [p["sizes"][size][robots]["singles_ms"] for p in parents
                        if robots in p["sizes"].get(size, {})]
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
