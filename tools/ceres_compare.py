#!/usr/bin/env python3
"""What the Ceres refinement kernels return, bit for bit, and how long they take: the tool that
shows a change of csrc/ceres_2d.hip, ceres_3d.hip or ceres_trust_region.h to be a refactor.

  python tools/ceres_compare.py [--library PATH] --out FILE
      runs, on the library named by --library (or CMX_SO_PATH, or the tree's own),
        * every 2D case of tests/ceres_edge_cases.py through the host grid and the resident grid,
        * every 3D case through cmx_ceres3d_match (intensity and Huber cases included) and the
          ones marked `resident` through cmx_ceres3d_match_grids,
        * the TSDF solves of tests/golden/ceres2d_tsdf_golden.npz (the failed initial evaluation
          and the failed candidates among them) on host and resident planes,
        * cmx_ceres2d_tsdf_residuals on the golden's residual fixtures,
        * one mixed batch through cmx_fast2d_refine_pairs and one through
          cmx_ceres3d_match_grids_batch,
      and writes one line per call: its name and every returned double as hex, with the step
      counts and the termination.
  python tools/ceres_compare.py --compare A B [--out FILE]
      the verdict on two such files (two libraries, two processes): one line.
  python tools/ceres_compare.py --time [--library PATH] --out FILE
      medians of --repeats calls (host clock, every call ends in a synchronise) of a 2D refinement
      of one 300-beam problem, of 64 in one cmx_fast2d_refine_pairs call, of a 3D refinement with
      two pairs, and of 64 of those in one cmx_ceres3d_match_grids_batch call: one JSON line.
  python tools/ceres_compare.py --summarise NEW PARENT PARENT PARENT [...] --out FILE
      both sets of medians, the parent runs' spread per shape, and whether the new medians lie
      within that spread of the parent's.
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for path in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    if path not in sys.path:
        sys.path.insert(0, path)

SHAPES = ("ceres2d_one_ms", "ceres2d_64_ms", "ceres3d_one_ms", "ceres3d_64_ms")


def _hex(values):
    return " ".join(float(v).hex() for v in np.asarray(values, np.float64).ravel())


def _line(name, pose, summary):
    return "%s pose %s cost %s %s steps %d %d termination %d" % (
        name, _hex(pose), float(summary["initial_cost"]).hex(), float(summary["final_cost"]).hex(),
        summary["num_successful_steps"], summary["num_unsuccessful_steps"], summary["termination"])


def _xyt(pose):
    return (pose.x, pose.y, pose.theta)


def _pose7(pose):
    return list(pose.translation) + list(pose.rotation)


class Scenes:
    """The scenes of tests/ceres_edge_cases.py with their grids on the host and in HBM."""

    def __init__(self):
        import ceres_edge_cases as ec
        from cartographer_amd import grid_2d, grid_3d, scan_matching as sm, scan_matching_3d as sm3
        from cartographer_amd import synth
        from oracle import pyoracle as orc
        synth.lib()
        orc.lib()
        self.ec, self.sm, self.sm3, self.synth, self.orc = ec, sm, sm3, synth, orc
        sc = ec.scene_2d(synth)
        lim = sc.lim
        self.host_2d = sm.Grid2D(sc.cells, lim["resolution"], lim["max_x"], lim["max_y"])
        self.resident_2d = grid_2d.ProbabilityGridOnDevice(
            ec.RES_2D, (lim["max_x"], lim["max_y"]), ec.NX_2D, ec.NY_2D, cells=sc.cells)
        sc3 = ec.scene_3d(synth)
        self.resident_3d = {}
        for resolution in (0.1, 0.2, 0.3):
            dev = grid_3d.HybridGridOnDevice(resolution)
            for origin, returns in sc3.inserts:
                dev.insert(origin, returns, 0.7, 0.4, 2)
            self.resident_3d[resolution] = dev

    def matcher_3d(self, case):
        return self.sm3.CeresScanMatcher3D(
            list(case.weights), case.translation_weight, case.rotation_weight,
            only_optimize_yaw=case.yaw_only, use_nonmonotonic_steps=case.nonmonotonic,
            max_num_iterations=case.iterations)

    def rigid3(self, init7):
        return self.sm3.Rigid3d(tuple(init7[:3]), tuple(init7[3:]))


def record(s):
    ec, sm, sm3 = s.ec, s.sm, s.sm3
    lines = []
    cases_2d = ec.cases_2d(s.synth)
    for case in cases_2d:
        w = case.weights
        m = sm.CeresScanMatcher2D(w[0], w[1], w[2], case.nonmonotonic, case.iterations)
        for where, grid in (("host", s.host_2d), ("resident", s.resident_2d)):
            pose, summary = m.match(case.target, sm.Rigid2d(*case.init), case.cloud, grid)
            lines.append(_line("2d/%s/%s" % (case.name, where), _xyt(pose), summary))
    cases_3d = ec.cases_3d(s.synth, s.orc)
    for case in cases_3d:
        m, init = s.matcher_3d(case), case.init7()
        pose, summary = m.match(case.target, s.rigid3(init), list(case.pairs))
        lines.append(_line("3d/%s/match" % case.name, _pose7(pose), summary))
        if case.resident:
            on_device = [(p[0], s.resident_3d[p[1]]) for p in case.pairs]
            pose, summary = m.match_grids(case.target, s.rigid3(init), on_device)
            lines.append(_line("3d/%s/match_grids" % case.name, _pose7(pose), summary))
    lines += record_tsdf(sm)
    # one mixed batch each: the picks of tests/test_gpu_ceres_edges.py, and every resident 3D case
    # with two pairs
    table = {c.name: c for c in cases_2d}
    picks = ["border_corner_minus_x_plus_y", "size_1", "border_all_outside_zero_gradient",
             "step_rejected_a_nonmonotonic", "size_257"]
    matcher = sm.FastCorrelativeScanMatcher2D(s.host_2d, 4)
    ceres = sm.CeresScanMatcher2D(5.0, 1.0, 1.0, True, 3)
    refined, summaries = ceres.refine_pairs(
        [matcher] * len(picks), [1, 1, 1, 1, 0], [sm.Rigid2d(*table[n].init) for n in picks],
        [table[n].cloud for n in picks])
    for name, pose, summary in zip(picks, refined, summaries):
        lines.append(_line("2d/refine_pairs/%s" % name, _xyt(pose), summary))
    two = [c for c in cases_3d if c.resident and len(c.pairs) == 2 and not c.yaw_only]
    ceres3 = sm3.CeresScanMatcher3D([1.0, 6.0], 5.0, 4e2, use_nonmonotonic_steps=True,
                                    max_num_iterations=12)
    poses, summaries = ceres3.match_grids_batch(
        [c.target for c in two], [s.rigid3(c.init7()) for c in two],
        [[(p[0], s.resident_3d[p[1]]) for p in c.pairs] for c in two])
    for case, pose, summary in zip(two, poses, summaries):
        lines.append(_line("3d/match_grids_batch/%s" % case.name, _pose7(pose), summary))
    return lines


def record_tsdf(sm):
    import make_ceres2d_tsdf_golden as mk
    from cartographer_amd import grid_2d
    golden = dict(np.load(os.path.join(ROOT, "tests", "golden", "ceres2d_tsdf_golden.npz")))
    insert_golden = dict(np.load(mk.INSERT_GOLDEN))
    lines = []
    for case in sorted({k.split("/")[1] for k in golden if k.startswith("solve/")}):
        key = "solve/" + case
        tsd, wgt, res, mx, my, trunc, maxw = mk.grid_of(golden, insert_golden,
                                                        str(golden[key + "/grid"]))
        cloud = mk.cloud_of(golden, insert_golden, key)
        o = golden[key + "/options"]
        m = sm.CeresScanMatcher2D(o[0], o[1], o[2], bool(o[3]), int(o[4]))
        grids = (("host", sm.TSDF2D(tsd, wgt, res, mx, my, trunc, maxw)),
                 ("resident", grid_2d.TSDF2DOnDevice(res, (mx, my), tsd.shape[1], tsd.shape[0],
                                                     trunc, maxw, tsd_cells=tsd, weight_cells=wgt)))
        for where, grid in grids:
            pose, summary = m.match(golden[key + "/target"], sm.Rigid2d(*golden[key + "/init"]),
                                    cloud, grid)
            lines.append(_line("tsdf/%s/%s" % (case, where), _xyt(pose), summary))
    for case in sorted({k.split("/")[1] for k in golden if k.startswith("res/")}):
        key = "res/" + case
        tsd, wgt, res, mx, my, trunc, maxw = mk.grid_of(golden, insert_golden,
                                                        str(golden[key + "/grid"]))
        grid = sm.TSDF2D(tsd, wgt, res, mx, my, trunc, maxw)
        poses, clouds = golden[key + "/poses"], golden[key + "/xyz"]
        for p in range(poses.shape[0]):
            valid, r, J = sm.tsdf_match_residuals(grid, float(golden[key + "/scaling"]), poses[p],
                                                  clouds[p])
            lines.append("tsdf_residuals/%s/%d valid %d%s" % (
                case, p, valid, " r %s J %s" % (_hex(r), _hex(J)) if valid else ""))
    return lines


def _median_ms(fn, repeats, warmup):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        times.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(times))


def measure(s, repeats, warmup):
    ec, sm, sm3 = s.ec, s.sm, s.sm3
    sc, sc3 = ec.scene_2d(s.synth), ec.scene_3d(s.synth)
    truth = sc.truth
    rng = np.random.default_rng(3)

    def near_2d():
        d = rng.uniform(-0.08, 0.08, 3) * (1.0, 1.0, 0.5)
        return sm.Rigid2d(float(truth[0] + d[0]), float(truth[1] + d[1]), float(truth[2] + d[2]))

    ceres = sm.CeresScanMatcher2D(20.0, 10.0, 1.0, False, 10)
    one = near_2d()
    matcher = sm.FastCorrelativeScanMatcher2D(s.host_2d, 4)
    many = [near_2d() for _ in range(64)]
    clouds = [sc.scan] * 64
    hi, lo = s.resident_3d[0.1], s.resident_3d[0.3]
    ceres3 = sm3.CeresScanMatcher3D([1.0, 6.0], 5.0, 4e2, max_num_iterations=12)

    def near_3d():
        t = np.asarray(sc3.pos) + rng.uniform(-0.06, 0.06, 3)
        yaw = ec.SCAN_YAW_3D + float(rng.uniform(-0.03, 0.03))
        half = 0.5 * yaw
        return sm3.Rigid3d(tuple(float(v) for v in t), (math.cos(half), 0.0, 0.0, math.sin(half)))

    one3 = near_3d()
    many3 = [near_3d() for _ in range(64)]
    entry = [(sc3.hi, hi), (sc3.lo, lo)]
    out = {"repeats": repeats, "points_2d": int(sc.scan.shape[0]),
           "points_3d": [int(sc3.hi.shape[0]), int(sc3.lo.shape[0])]}
    out["ceres2d_one_ms"] = _median_ms(
        lambda: ceres.match(_xyt(one)[:2], one, sc.scan, s.resident_2d), repeats, warmup)
    out["ceres2d_64_ms"] = _median_ms(
        lambda: ceres.refine_pairs([matcher] * 64, None, many, clouds), repeats, warmup)
    out["ceres3d_one_ms"] = _median_ms(
        lambda: ceres3.match_grids(one3.translation, one3, entry), repeats, warmup)
    out["ceres3d_64_ms"] = _median_ms(
        lambda: ceres3.match_grids_batch([p.translation for p in many3], many3, [entry] * 64),
        repeats, warmup)
    return out


def compare(a_path, b_path):
    with open(a_path) as f:
        a = f.read().splitlines()
    with open(b_path) as f:
        b = f.read().splitlines()
    differing = [x.split(" ", 1)[0] for x, y in zip(a, b) if x != y]
    if len(a) != len(b) or differing:
        return "DIFFERENT: %d and %d calls, %d differ: %s" % (len(a), len(b), len(differing),
                                                              " ".join(differing[:10]))
    return "identical: %d calls, every returned double, step count and termination" % len(a)


def summarise(new_path, parent_paths):
    def load(path):
        with open(path) as f:
            return json.loads(f.read())
    new, parents = load(new_path), [load(p) for p in parent_paths]
    out = {"new": new, "parent_runs": parents, "shapes": {}}
    for shape in SHAPES:
        runs = [p[shape] for p in parents]
        spread = max(runs) - min(runs)
        out["shapes"][shape] = {
            "new": new[shape], "parent": runs, "parent_spread_ms": spread,
            "within_spread": bool(min(runs) - spread <= new[shape] <= max(runs) + spread)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--library", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--compare", nargs=2, default=None)
    ap.add_argument("--summarise", nargs="+", default=None)
    args = ap.parse_args()
    if args.compare:
        text = compare(*args.compare)
    elif args.summarise:
        text = json.dumps(summarise(args.summarise[0], args.summarise[1:]))
    else:
        if args.library:
            os.environ["CMX_SO_PATH"] = os.path.abspath(args.library)
        from cartographer_amd import _lib
        assert _lib.lib().cmx_device_count() >= 1, "no HIP device"
        scenes = Scenes()
        if args.time:
            out = measure(scenes, args.repeats, args.warmup)
            out["library"] = os.path.relpath(_lib.SO_PATH, ROOT)
            text = json.dumps(out)
        else:
            text = "\n".join(record(scenes))
    print(text if len(text) < 4000 else "%d lines" % len(text.splitlines()))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
