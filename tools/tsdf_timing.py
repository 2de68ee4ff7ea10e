#!/usr/bin/env python3
"""Timing of the device-resident TSDF2D (cartographer_amd/csrc/tsdf_2d.hip); prints one JSON line.

Legs (each after warm-up, median over --calls calls, host clock around the call; every call ends
in a synchronise):
  insert_lua_ms / insert_free_space_ms   cmx_tsdf2d_insert of one ~1000-point room scan
                                         (tests/golden/tsdf_insert_golden.npz inputs) into a grid
                                         that already holds the room, lua defaults / free space on
  ref_cpu_insert_*_ms                    the reference's own inserter (oracle/_ref) on this host,
                                         same scans (null where oracle/_ref is not built)
  rt_match_resident_ms / rt_match_host_planes_ms
                                         cmx_rt2d_match_tsdf_grid against cmx_rt2d_match_tsdf
                                         (planes uploaded per call) on a 200x200 grid
  cells_changed_per_insert_*             cells whose (tsd, weight) the insert changed (median)
  ceres_tsdf_resident_ms / ceres_tsdf_host_planes_ms
                                         CeresScanMatcher2D::Match on the same TSDF (lua local
                                         options 1 / 10 / 40, 20 iterations) of one ~1000-point
                                         room scan: cmx_ceres2d_match_tsdf_grid against
                                         cmx_ceres2d_match_tsdf (planes uploaded per call)
  refine_batch_tsdf_64_ms                cmx_ceres2d_refine_batch_tsdf of 64 (pose, grid) pairs
                                         (pose_graph.lua's constraint-builder options)
  standin_cpu_ceres_tsdf_ms              the same solve by the reference's cost function over the
                                         STAND-IN solver of oracle/ref_shims/ceres (not Ceres), on
                                         this host; null where the reference tree is absent
  batch_<N>: (N = 128, 1024; --batch, --sizes) N distinct (grid, scan, pose) triples on 200x200
             grids, the whole ~1000-point room scans (less a tail of up to 30 points), the window
             of rt_match_*:
    bulk_ms / legacy_ms     cmx_rt2d_match_tsdf_grid_batch on the integer bulk path (debug switch
                            rt2d_tsdf_batch_bulk) and on the per-candidate batch kernels
                            (rt2d_tsdf_batch_legacy: what the entry runs by default)
    sequential_ms           N sequential cmx_rt2d_match_tsdf_grid calls on the same inputs
    baseline_sequential_ms  the same loop through another build of the library
                            (--baseline-lib: the parent commit's), in this process, on this box
    each with its minimum and maximum over the calls (the run-to-run spread)
Usage: python tools/tsdf_timing.py [--calls 60] [--batch] [--sizes 128,1024]
                                   [--baseline-lib PATH] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))


def _median_ms(fn, calls, warmup=5):
    for k in range(warmup):
        fn(k)
    times = []
    for k in range(calls):
        t0 = time.perf_counter()
        fn(k)
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times))


def _ceres_legs(out, dev, host, cloud, calls):
    from cartographer_amd import scan_matching as sm
    local = sm.CeresScanMatcher2D(1.0, 10.0, 40.0, False, 20)
    init = sm.Rigid2d(0.03, -0.02, 0.015)
    target = [init.x, init.y]
    out["ceres_tsdf_points"] = int(cloud.shape[0])
    out["ceres_tsdf_resident_ms"] = _median_ms(lambda k: local.match(target, init, cloud, dev),
                                               calls)
    out["ceres_tsdf_host_planes_ms"] = _median_ms(lambda k: local.match(target, init, cloud, host),
                                                  calls)
    a, b = local.match(target, init, cloud, dev), local.match(target, init, cloud, host)
    out["ceres_tsdf_equal"] = bool(a == b)
    out["ceres_tsdf_summary"] = a[1]
    constraint = sm.CeresScanMatcher2D(20.0, 10.0, 1.0, True, 10)
    rng = np.random.default_rng(3)
    poses = [sm.Rigid2d(*rng.uniform(-0.04, 0.04, 3)) for _ in range(64)]
    out["refine_batch_tsdf_64_ms"] = _median_ms(
        lambda k: constraint.refine_batch_tsdf([dev] * 64, None, poses, cloud), calls)
    # The driver compiles against the reference's headers: without the tree the leg is null
    # (not measured); with it, any failure of the leg is an error.
    out["standin_cpu_ceres_tsdf_ms"] = None
    if os.path.isdir("/root/reference"):
        import make_ceres2d_tsdf_golden as mc
        L = mc._driver()
        grid = (host.cells, host.weight_cells, host.resolution, host.max_x, host.max_y,
                host.truncation_distance, host.max_weight)
        opts = (1.0, 10.0, 40.0, 0.0, 20.0)
        out["standin_cpu_ceres_tsdf_ms"] = _median_ms(
            lambda k: mc.ref_match(L, grid, opts, target, [init.x, init.y, init.theta], cloud),
            calls)


def _spread_ms(fn, calls, warmup=3):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return dict(median=float(np.median(times)), min=float(np.min(times)),
                max=float(np.max(times)), calls=calls)


def _batch_legs(out, scans, make_grid, opts, calls, baseline_lib, sizes=(128, 1024)):
    """The batch entry against sequential single calls (this build and, with --baseline-lib,
    another build of the library) on the same N distinct triples."""
    import ctypes as C
    from cartographer_amd import _lib, scan_matching as sm
    rt = sm.RealTimeCorrelativeScanMatcher2D(0.3, np.deg2rad(8.0), 0.1, 0.1)
    grids = []
    for g in range(16):                               # 16 grids, each from its own subset of scans
        dev = make_grid()
        for k in range(12):
            if (k + g) % 4 != 3:
                dev.insert(scans[k][0], scans[k][1], **opts)
        grids.append(dev)
    base = None
    if baseline_lib:
        base = C.CDLL(baseline_lib)
        base_grids = []
        for dev in grids:
            host = dev.to_host()
            lim = _lib.Grid2DLimits(host.resolution, host.max_x, host.max_y, host.cells.shape[1],
                                    host.cells.shape[0], 0.0, 0.0)
            h = C.c_void_p()
            base.cmx_tsdf2d_create.argtypes = _lib.lib().cmx_tsdf2d_create.argtypes
            base.cmx_rt2d_match_tsdf_grid.argtypes = _lib.lib().cmx_rt2d_match_tsdf_grid.argtypes
            assert base.cmx_tsdf2d_create(C.byref(lim), host.truncation_distance, host.max_weight,
                                          host.cells.ctypes.data, host.weight_cells.ctypes.data,
                                          0, C.byref(h)) == 0
            base_grids.append(h)
    rng = np.random.default_rng(7)
    for num in sizes:
        which, clouds, inits = [], [], []
        for m in range(num):
            o, r = scans[m % 12]
            # the whole ~1000-point scan less a tail of 0 ... 30 points (counts that are not all
            # multiples of 64); grid, scan, count and the random pose make the triple distinct
            scan = np.ascontiguousarray(r[: len(r) - m % 31] -
                                        np.array([o[0], o[1], 0.0], np.float32))
            which.append(m % 16)
            clouds.append(scan)
            inits.append([float(o[0]) + rng.uniform(-0.06, 0.06),
                          float(o[1]) + rng.uniform(-0.06, 0.06), rng.uniform(-0.03, 0.03)])
        batch = sm.Rt2DBatch(rt, [grids[g] for g in which], clouds)
        init = np.array(inits)
        leg = {"points_per_scan": float(np.mean([c.shape[0] for c in clouds]))}
        _lib.debug_set(rt2d_tsdf_batch_bulk=1)
        bulk = batch.match(init)
        bulk_scores, bulk_poses = bulk[0].copy(), bulk[1].copy()
        leg["bulk_stats"] = {k: bulk[2][k] for k in ("candidates_scored", "refined_candidates",
                                                      "finalists")}
        leg["bulk_ms"] = _spread_ms(lambda: batch.match(init), calls)
        _lib.debug_set(rt2d_tsdf_batch_legacy=1)
        legacy = batch.match(init)
        leg["bulk_equals_legacy"] = bool(np.array_equal(legacy[0], bulk_scores) and
                                         np.array_equal(legacy[1], bulk_poses))
        leg["legacy_ms"] = _spread_ms(lambda: batch.match(init), calls)
        _lib.debug_reset()
        poses_c = [sm.Rigid2d(*p).to_c() for p in inits]
        score, pose, stats = C.c_double(), _lib.Pose2d(), _lib.MatchStats()

        def sequential(L, handles):
            for m in range(num):
                L.cmx_rt2d_match_tsdf_grid(C.byref(rt.options), handles[which[m]],
                                           C.byref(poses_c[m]), clouds[m].ctypes.data,
                                           clouds[m].shape[0], C.byref(score), C.byref(pose),
                                           C.byref(stats))
        seq_calls = max(20, calls // 3) if num <= 128 else 20
        leg["sequential_ms"] = _spread_ms(
            lambda: sequential(_lib.lib(), [g._h for g in grids]), seq_calls)
        leg["baseline_sequential_ms"] = None if base is None else _spread_ms(
            lambda: sequential(base, base_grids), seq_calls)
        out[f"batch_{num}"] = leg


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=60)
    ap.add_argument("--batch", action="store_true", help="only the batch_<N> legs")
    ap.add_argument("--baseline-lib", default=None,
                    help="libcartographer_mi355x.so of another build (the parent commit's)")
    ap.add_argument("--sizes", default="128,1024", help="batch sizes of the batch_<N> legs")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    import make_tsdf_insert_golden as mk
    from cartographer_amd import grid_2d, scan_matching as sm
    golden = dict(np.load(os.path.join(ROOT, "tests", "golden", "tsdf_insert_golden.npz")))
    scans = [mk.step_inputs(golden, "room_lua", k)[:2] for k in range(12)]
    out = {"points_per_scan": float(np.mean([r.shape[0] for _, r in scans]))}
    res, mx, my, _, _, t, w = golden["room_lua/meta"]
    # 200 x 200 cells of 5 cm over the room's points: no insert grows the grid
    pts = np.concatenate([r for _, r in scans] + [o[None] for o, _ in scans])
    lo, hi = pts.min(0), pts.max(0)
    assert (hi - lo)[:2].max() < 9.0, "the room does not fit 200 x 200 cells"
    margin = (10.0 - (hi - lo)) / 2
    centre = (float(hi[0] + margin[0]), float(hi[1] + margin[1]))
    try:
        from oracle import pyoracle as orc
        ref = orc if orc.ref_lib() is not None else None
    except Exception:  # pragma: no cover - the oracle is optional here
        ref = None
    if args.batch:
        from cartographer_amd import grid_2d as g2
        out = {"calls": args.calls}
        _batch_legs(out, scans, lambda: g2.TSDF2DOnDevice(res, centre, 200, 200, t, w),
                    mk.LUA_DEFAULTS, args.calls, args.baseline_lib,
                    tuple(int(v) for v in args.sizes.split(",")))
        line = json.dumps(out, sort_keys=True)
        print(line)
        if args.out:
            with open(args.out, "w") as f:
                f.write(line + "\n")
        return
    for label, opts in (("lua", mk.LUA_DEFAULTS),
                        ("free_space", dict(mk.LUA_DEFAULTS, update_free_space=True))):
        dev = grid_2d.TSDF2DOnDevice(res, centre, 200, 200, t, w)
        for o, r in scans:
            dev.insert(o, r, **opts)
        assert dev.limits["num_x_cells"] == 200, "the timing grid grew"
        out[f"insert_{label}_ms"] = _median_ms(
            lambda k: dev.insert(scans[k % 12][0], scans[k % 12][1], **opts), args.calls)
        changed = []
        for k in range(12):
            a = dev.planes()
            dev.insert(scans[k][0], scans[k][1], **opts)
            b = dev.planes()
            changed.append(int(np.count_nonzero((a[0] != b[0]) | (a[1] != b[1]))))
        out[f"cells_changed_per_insert_{label}"] = float(np.median(changed))
        if ref is not None:
            g = ref.ReferenceTSDF2D(res, centre, 200, 200, t, w)
            for o, r in scans:
                g.insert(o, r, **opts)
            out[f"ref_cpu_insert_{label}_ms"] = _median_ms(
                lambda k: g.insert(scans[k % 12][0], scans[k % 12][1], **opts), args.calls)
        else:
            out[f"ref_cpu_insert_{label}_ms"] = None
        if label == "lua":
            host = dev.to_host()
            rt = sm.RealTimeCorrelativeScanMatcher2D(0.3, np.deg2rad(8.0), 0.1, 0.1)
            o, r = scans[3]
            scan = r[::2] - np.array([o[0], o[1], 0.0], np.float32)
            init = sm.Rigid2d(float(o[0]) + 0.05, float(o[1]) - 0.04, 0.02)
            out["rt_match_points"] = int(scan.shape[0])
            out["rt_match_resident_ms"] = _median_ms(lambda k: rt.match(init, scan, dev),
                                                     args.calls)
            out["rt_match_host_planes_ms"] = _median_ms(lambda k: rt.match(init, scan, host),
                                                        args.calls)
            a, b = rt.match(init, scan, dev), rt.match(init, scan, host)
            out["rt_match_equal"] = bool(a[0] == b[0] and a[1].x == b[1].x and a[1].y == b[1].y
                                         and a[1].theta == b[1].theta)
            _ceres_legs(out, dev, host, r, args.calls)
    out["calls"] = args.calls
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
