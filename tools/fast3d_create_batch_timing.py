#!/usr/bin/env python3
"""Timing of the fast-3D matchers of many submaps built in one call (cmx_fast3d_create_batch)
against one constructor call per submap; prints one JSON line and writes it to --out.

N in --sizes (default 1, 32, 256) distinct C5-sized submaps (tools/fast3d_create_timing.py's: a
15 x 15 x 7.5 m room at 0.10 m / 0.45 m from eight 32 x 512 sweeps, seeds 42, 43, ...),
pose_graph.lua's options (depth 8, full-resolution depth 3), 120-bin histograms: the shape of a
loaded 3D map, or of a node's first global constraint against every finished submap.  Sources are
grids resident in HBM ("grid") and their voxel lists in host memory ("voxels": downloaded before
anything is timed).  Legs, per N and kind of source (host clock around the creates and the
destroys of all N matchers; every create ends in a synchronise and every destroy frees device
memory, which waits for the device; median, min and max over --repeats after --warmup;
"*_create_ms" is the part up to the last create):
  batch_<kind>_ms     one cmx_fast3d_create_batch call
  singles_<kind>_ms   N cmx_fast3d_create_from_grids / cmx_fast3d_create calls
Before anything is timed, every level of the batch-built matchers is compared with the single
creates' ("levels_equal").
Of the batch call the debug switch host_trace reports, per call (medians over five calls, in
microseconds of the host's clock): bounds (the voxel-list plans, the one launch that finds the
boxes of the resident sources with its synchronisation, the plans from them), alloc (the N
device allocations), stage (tables and voxel lists into the pinned block), issue (the copy and
the launches), wait (the synchronisations at the chains' ends), and the launches and chains
counted on the host.
gpu_max_hw_queues is GPU_MAX_HW_QUEUES as the process sees it once the library is loaded.
--library PATH loads another build of the library (the parent commit's, for the yardstick on
the same box): only the singles legs are measured.  --yardstick F [F ...] takes such runs' JSON
(before and after this one) and records their figures, their spread and the ratios to this
run's batch legs; with --merge F nothing is measured: F is an earlier run of this tree.
Writes profiles/fast3d_create_batch_timing.json unless --out names another file.
Usage: python tools/fast3d_create_batch_timing.py [--sizes 1 32 256] [--repeats 20] [--warmup 3]
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
DEPTH, FRD = 8, 3
KINDS = ("grid", "voxels")


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
    ap.add_argument("--sizes", type=int, nargs="*", default=[1, 32, 256])
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--library", default=None)
    ap.add_argument("--yardstick", nargs="*", default=[])
    ap.add_argument("--merge", default=None)
    ap.add_argument("--out",
                    default=os.path.join(ROOT, "profiles", "fast3d_create_batch_timing.json"))
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
            for kind in KINDS:
                for part in ("", "_create"):
                    key = f"singles_{kind}{part}_ms"
                    runs = [p["n"][str(n)][key] for p in parents if str(n) in p["n"]]
                    if not runs:
                        continue
                    mean = float(np.mean(runs))
                    row = out["n"][str(n)]
                    batch = row[f"batch_{kind}{part}_ms"]
                    row[f"parent_{key}"] = runs
                    row[f"parent_singles_{kind}{part}_spread"] = (max(runs) - min(runs)) / mean
                    row[f"parent_singles_{kind}{part}_over_batch"] = mean / batch
                    # the batch wins where it is below the parent by more than the parent's own
                    # spread
                    row[f"batch_{kind}{part}_beats_parent"] = \
                        bool(min(runs) - batch > max(runs) - min(runs))
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


def _submap(synth, grid_3d, seed):
    """The resident grids of tools/fast3d_create_timing.py's submap for `seed`."""
    world = synth.World3D(seed, (15.0, 15.0, 7.5))
    high, low = grid_3d.HybridGridOnDevice(0.1), grid_3d.HybridGridOnDevice(0.45)
    for p in range(8):                     # synth.make_submap_3d(seed, ..., 8, 32, 512)
        pos = world.free_position(seed * 1009 + p, 0.5)
        yaw = 0.37 * p
        sensor = world.scan(pos, yaw, 32, 512, seed=seed * 31 + p).astype(np.float64)
        c, s = np.cos(yaw), np.sin(yaw)
        in_map = np.stack([pos[0] + c * sensor[:, 0] - s * sensor[:, 1],
                           pos[1] + s * sensor[:, 0] + c * sensor[:, 1],
                           pos[2] + sensor[:, 2]], 1).astype(np.float32)
        for g in (high, low):
            g.insert(pos.astype(np.float32), in_map, 0.7, 0.4, 2)
    return high, low


def measure(args):
    if args.library:
        os.environ["CMX_SO_PATH"] = os.path.abspath(args.library)
    from cartographer_amd import _lib, grid_3d, synth
    L = _lib.lib()
    has_batch = hasattr(L, "cmx_fast3d_create_batch")
    most = max(args.sizes)
    options = _lib.Fast3DOptions(DEPTH, FRD, 0.77, 0.55, 5.0, 1.0, math.radians(15.0))
    grids, lists, hists = [], [], []
    for k in range(most):
        high, low = _submap(synth, grid_3d, 42 + k)
        grids.append((high, low))
        lists.append((np.ascontiguousarray(high.voxels(), _lib.VOXEL_DTYPE), high.grid_size,
                      np.ascontiguousarray(low.voxels(), _lib.VOXEL_DTYPE)))
        hists.append(np.random.default_rng(1 + k).uniform(0.0, 1.0, 120).astype(np.float32))
    handles = (C.c_void_p * most)()
    destroy = L.cmx_fast3d_destroy
    sources = {}
    if has_batch:
        for kind in KINDS:
            sources[kind] = (_lib.Fast3DSource * most)()
            for k in range(most):
                s = sources[kind][k]
                if kind == "grid":
                    s.high_resolution_grid, s.low_resolution_grid = grids[k][0]._h, grids[k][1]._h
                else:
                    s.resolution, s.grid_size, s.low_resolution = 0.1, lists[k][1], 0.45
                    s.voxels, s.num_voxels = lists[k][0].ctypes.data, len(lists[k][0])
                    s.low_resolution_voxels = lists[k][2].ctypes.data
                    s.num_low_resolution_voxels = len(lists[k][2])
                s.rotational_scan_matcher_histogram, s.histogram_size = hists[k].ctypes.data, 120

    def finish(n, t0):
        t1 = time.perf_counter()
        for k in range(n):
            destroy(handles[k])
            handles[k] = None
        return 1e3 * (t1 - t0), 1e3 * (time.perf_counter() - t0)

    def batch(kind, n, keep=False):
        t0 = time.perf_counter()
        _lib.check(L.cmx_fast3d_create_batch(C.byref(options), sources[kind], n, 0, handles))
        return None if keep else finish(n, t0)

    def singles(kind, n, keep=False):
        h = C.c_void_p()
        t0 = time.perf_counter()
        for k in range(n):
            if kind == "grid":
                _lib.check(L.cmx_fast3d_create_from_grids(
                    C.byref(options), grids[k][0]._h, grids[k][1]._h, hists[k].ctypes.data, 120,
                    C.byref(h)))
            else:
                vox, grid_size, low = lists[k]
                _lib.check(L.cmx_fast3d_create(
                    C.byref(options), 0.1, grid_size, vox.ctypes.data, len(vox), 0.45,
                    low.ctypes.data, len(low), hists[k].ctypes.data, 120, 0, C.byref(h)))
            handles[k] = h.value
        return None if keep else finish(n, t0)

    def levels(n):
        """Every level of the n matchers in `handles`, then destroyed."""
        got = []
        lo, dims = np.zeros(3, np.int32), np.zeros(3, np.int32)
        for k in range(n):
            for level in range(DEPTH):
                _lib.check(L.cmx_fast3d_level_info(handles[k], level, lo.ctypes.data,
                                                   dims.ctypes.data))
                a = np.empty((dims[2], dims[1], dims[0]), np.uint8)
                _lib.check(L.cmx_fast3d_level_cells(handles[k], level, a.ctypes.data))
                got += [lo.copy(), a]
            destroy(handles[k])
            handles[k] = None
        return got

    out = dict(sizes=list(args.sizes),
               submap="15 x 15 x 7.5 m at 0.10 / 0.45 m, eight 32 x 512 sweeps",
               high_voxels=[len(v[0]) for v in lists[:4]], low_voxels=[len(v[2]) for v in lists[:4]],
               depth=DEPTH, full_resolution_depth=FRD, repeats=args.repeats, warmup=args.warmup,
               library="this tree" if not args.library else "other build",
               device=_device_name(), gpu_max_hw_queues=_getenv("GPU_MAX_HW_QUEUES"), n={})
    if has_batch:
        check = min(4, most)
        singles("grid", check, keep=True)
        want = levels(check)
        equal = True
        for kind in KINDS:
            batch(kind, check, keep=True)
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

        for kind in KINDS:
            leg(f"singles_{kind}_ms", lambda: singles(kind, n))
        if has_batch:
            for kind in KINDS:
                leg(f"batch_{kind}_ms", lambda: batch(kind, n))
                row[f"singles_{kind}_over_batch"] = row[f"singles_{kind}_ms"] / \
                    row[f"batch_{kind}_ms"]
                # where the call's time goes: host_trace writes one line per call
                _lib.debug_set(host_trace=1)
                try:
                    text = _captured_stderr(lambda: [batch(kind, n) for _ in range(5)])
                finally:
                    _lib.debug_reset()
                found = re.findall(r"fast3d_create_batch matchers=(\d+) chains=(\d+) "
                                   r"launches=(\d+) bounds=(\d+) alloc=(\d+) stage=(\d+) "
                                   r"issue=(\d+) wait=(\d+)", text)
                if found:
                    cols = np.array(found, np.float64)
                    row[f"batch_{kind}_trace"] = dict(
                        chains=int(cols[0, 1]), launches=int(cols[0, 2]),
                        bounds_us=float(np.median(cols[:, 3])),
                        alloc_us=float(np.median(cols[:, 4])),
                        stage_us=float(np.median(cols[:, 5])),
                        issue_us=float(np.median(cols[:, 6])),
                        wait_us=float(np.median(cols[:, 7])))
        out["n"][str(n)] = row
    return out


if __name__ == "__main__":
    main()
