#!/usr/bin/env python3
"""Timing of the fast-2D matchers of many submaps built in one call (cmx_fast2d_create_batch)
against one constructor call per submap; prints one JSON line and writes it to --out.

N in --sizes (default 1, 32, 512) distinct 400 x 400 submaps at 0.05 m from 30 scans each,
pose_graph.lua's options (depth 7, windows 7 m / 30 deg): the shape of a loaded map, or of a
node's first global constraint against every finished submap.  Sources are host cells ("host")
and grids resident in HBM ("grid").  Legs, per N and kind of source (host clock around the
creates and the destroys of all N matchers; every create ends in a synchronise and every
destroy frees device memory, which waits for the device; median, min and max over --repeats
after --warmup; "*_create_ms" is the part up to the last create):
  batch_<kind>_ms     one cmx_fast2d_create_batch call
  singles_<kind>_ms   N cmx_fast2d_create / cmx_fast2d_create_from_grid calls
Before anything is timed, every level of the batch-built matchers is compared with the single
creates' at the timed size ("levels_equal").
Of the batch call the debug switch host_trace reports, per call (medians over five calls, in
microseconds of the host's clock): alloc (the N device allocations and the host-side layout),
stage (tables and host cells into the pinned block), issue (the copy and the launches), wait
(the synchronisations), and the launches and chains counted on the host.
gpu_max_hw_queues is GPU_MAX_HW_QUEUES as the process sees it once the library is loaded.
--library PATH loads another build of the library (the parent commit's, for the yardstick on
the same box): only the singles legs are measured.  --yardstick F [F ...] takes such runs' JSON
(before and after this one) and records their figures, their spread and the ratios to this
run's batch legs; with --merge F nothing is measured: F is an earlier run of this tree.
Writes profiles/fast2d_create_batch_timing.json unless --out names another file.
Usage: python tools/fast2d_create_batch_timing.py [--sizes 1 32 512] [--repeats 20] [--warmup 3]
                                                  [--library PATH] [--yardstick F ...]
                                                  [--merge F] [--out F]
"""
import argparse
import ctypes as C
import json
import math
import os
import re
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEPTH, LIN, ANG = 7, 7.0, math.radians(30.0)


def _timed(fn, repeats, warmup):
    """fn() -> (ms up to the last create, ms in all); medians and the range of the total."""
    for _ in range(warmup):
        fn()
    create, total = [], []
    for _ in range(repeats):
        a, b = fn()
        create.append(a)
        total.append(b)
    return dict(median=float(np.median(total)), min=float(min(total)), max=float(max(total)),
                create=float(np.median(create)))


def _device_name():
    hip = C.CDLL("libamdhip64.so")
    name = C.create_string_buffer(256)
    if hip.hipDeviceGetName(name, 256, 0) != 0:
        return "unknown"
    return name.value.decode() or "unknown"


def _getenv(name):
    getenv = C.CDLL(None).getenv
    getenv.restype = C.c_char_p
    value = getenv(name.encode())
    return None if value is None else value.decode()


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[1, 32, 512])
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--library", default=None)
    ap.add_argument("--yardstick", nargs="*", default=[])
    ap.add_argument("--merge", default=None)
    ap.add_argument("--out",
                    default=os.path.join(ROOT, "profiles", "fast2d_create_batch_timing.json"))
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
        for n in out["sizes"]:
            for kind in ("host", "grid"):
                key = f"singles_{kind}_ms"
                runs = [p["n"][str(n)][key] for p in parents if str(n) in p["n"]]
                if not runs:
                    continue
                mean = float(np.mean(runs))
                row = out["n"][str(n)]
                row[f"parent_{key}"] = runs
                row[f"parent_singles_{kind}_spread"] = (max(runs) - min(runs)) / mean
                row[f"parent_singles_{kind}_over_batch"] = mean / row[f"batch_{kind}_ms"]
                # the batch wins where it is below the parent by more than the parent's own spread
                row[f"batch_{kind}_beats_parent"] = \
                    bool(min(runs) - row[f"batch_{kind}_ms"] > max(runs) - min(runs))
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
    has_batch = hasattr(L, "cmx_fast2d_create_batch")
    most = max(args.sizes)
    options = _lib.Fast2DOptions(LIN, ANG, DEPTH)
    cells, limits, grids = [], [], []
    for k in range(most):
        c, lim, _ = synth.make_submap(1000 + k, 400, 400, 0.05, 30, 1000, 10.0, 0.01)
        cells.append(np.ascontiguousarray(c, np.uint16))
        limits.append(_lib.Grid2DLimits(0.05, lim["max_x"], lim["max_y"], 400, 400, 0.1, 0.9))
        grids.append(grid_2d.ProbabilityGridOnDevice(0.05, (lim["max_x"], lim["max_y"]), 400, 400,
                                                     c))
    host_sources = (_lib.Fast2DSource * most)()
    grid_sources = (_lib.Fast2DSource * most)()
    for k in range(most):
        host_sources[k].limits = C.pointer(limits[k])
        host_sources[k].cells = cells[k].ctypes.data
        grid_sources[k].grid = grids[k]._h
    handles = (C.c_void_p * most)()
    destroy = L.cmx_fast2d_destroy

    def finish(n, t0):
        t1 = time.perf_counter()
        for k in range(n):
            destroy(handles[k])
            handles[k] = None
        return 1e3 * (t1 - t0), 1e3 * (time.perf_counter() - t0)

    def batch(sources, n, keep=False):
        t0 = time.perf_counter()
        _lib.check(L.cmx_fast2d_create_batch(C.byref(options), sources, n, 0, handles))
        return None if keep else finish(n, t0)

    def singles_host(n, keep=False):
        h = C.c_void_p()
        t0 = time.perf_counter()
        for k in range(n):
            _lib.check(L.cmx_fast2d_create(C.byref(options), C.byref(limits[k]),
                                           cells[k].ctypes.data, 0, C.byref(h)))
            handles[k] = h.value
        return None if keep else finish(n, t0)

    def singles_grid(n, keep=False):
        h = C.c_void_p()
        t0 = time.perf_counter()
        for k in range(n):
            _lib.check(L.cmx_fast2d_create_from_grid(C.byref(options), grids[k]._h, C.byref(h)))
            handles[k] = h.value
        return None if keep else finish(n, t0)

    def levels(n):
        """Every level of the n matchers in `handles`, then destroyed."""
        got = []
        wx, wy = C.c_int32(), C.c_int32()
        for k in range(n):
            for level in range(DEPTH):
                _lib.check(L.cmx_fast2d_level_dims(handles[k], level, C.byref(wx), C.byref(wy)))
                a = np.empty((wy.value, wx.value), np.uint8)
                _lib.check(L.cmx_fast2d_level_cells(handles[k], level, a.ctypes.data))
                got.append(a)
            destroy(handles[k])
            handles[k] = None
        return got

    out = dict(sizes=list(args.sizes), submap="400x400 at 0.05 m, 30 scans", depth=DEPTH,
               repeats=args.repeats, warmup=args.warmup,
               library="this tree" if not args.library else "other build",
               device=_device_name(), gpu_max_hw_queues=_getenv("GPU_MAX_HW_QUEUES"), n={})
    if has_batch:
        check = min(32, most)                      # the timed size (the shape is the same at 512)
        singles_host(check, keep=True)
        want = levels(check)
        equal = True
        for sources in (host_sources, grid_sources):
            batch(sources, check, keep=True)
            got = levels(check)
            equal = equal and len(got) == len(want) and all(
                np.array_equal(a, b) for a, b in zip(got, want))
        out["levels_equal"] = bool(equal)
        out["levels_compared"] = check
        if not equal:
            raise SystemExit("batch-built levels differ from the single creates': nothing timed")
    for n in args.sizes:
        row = {}

        def leg(name, fn):
            t = _timed(fn, args.repeats, args.warmup)
            row[name] = t["median"]
            row[name.replace("_ms", "_min_max_ms")] = [t["min"], t["max"]]
            row[name.replace("_ms", "_create_ms")] = t["create"]

        leg("singles_host_ms", lambda: singles_host(n))
        leg("singles_grid_ms", lambda: singles_grid(n))
        if has_batch:
            for kind, sources in (("host", host_sources), ("grid", grid_sources)):
                leg(f"batch_{kind}_ms", lambda: batch(sources, n))
                row[f"singles_{kind}_over_batch"] = row[f"singles_{kind}_ms"] / \
                    row[f"batch_{kind}_ms"]
                # where the call's time goes: host_trace writes one line per call
                _lib.debug_set(host_trace=1)
                try:
                    text = _captured_stderr(lambda: [batch(sources, n) for _ in range(5)])
                finally:
                    _lib.debug_reset()
                found = re.findall(r"fast2d_create_batch matchers=(\d+) chains=(\d+) "
                                   r"launches=(\d+) alloc=(\d+) stage=(\d+) issue=(\d+) "
                                   r"wait=(\d+)", text)
                if found:
                    cols = np.array(found, np.float64)
                    row[f"batch_{kind}_trace"] = dict(
                        chains=int(cols[0, 1]), launches=int(cols[0, 2]),
                        alloc_us=float(np.median(cols[:, 3])),
                        stage_us=float(np.median(cols[:, 4])),
                        issue_us=float(np.median(cols[:, 5])),
                        wait_us=float(np.median(cols[:, 6])))
        out["n"][str(n)] = row
    return out


if __name__ == "__main__":
    main()
