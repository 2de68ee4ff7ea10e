#!/usr/bin/env python3
"""Generates tests/golden/tsdf_insert_golden.npz: TSDF2D planes and limits after every insert of
the scenarios below, made by the REFERENCE'S OWN TSDFRangeDataInserter2D / normal_estimation_2d /
TSDF2D sources (oracle/_ref, compiled unmodified against the stand-in headers of
oracle/ref_shims), for tests/test_gpu_tsdf.py.  The inputs (origins, returns, options) are stored
with the results, so the GPU box needs neither the reference nor the oracle.

Scenarios:
  ref_*     the eight tests of tsdf_range_data_inserter_2d_test.cc (their 8x1 grid, their options)
  room_*    a 16x16 grid grown by twelve ~1000-point scans of a synthetic room, three option sets
  edges     dense beams, duplicate points, hits inside the truncation distance, an angle kernel
            narrow enough that weights underflow to 0, an empty insert (that grows the grid)

Key layout: "<scenario>/meta" (resolution, max_x, max_y, nx, ny, truncation, max_weight),
"<scenario>/<step>/{origin,returns,options,repeat}" and "<scenario>/<step>/{limits,digest}" (the
state after the step; `repeat` inserts of the same range data; `digest` = sha256 of the tsd then
the weight plane's bytes).  The planes themselves ("/tsd", "/weight") are stored for every step
of the small scenarios and for the last step of the room ones; room scenarios after the first
name the step whose returns they share ("/returns_of") instead of storing them again.  Usage:
    python tests/golden/make_tsdf_insert_golden.py
"""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

OPTION_KEYS = ("truncation_distance", "maximum_weight", "update_free_space", "num_normal_samples",
               "sample_radius", "project_sdf_distance_to_scan_normal",
               "update_weight_range_exponent", "angle_kernel_bandwidth",
               "distance_kernel_bandwidth")

# RangeDataInserterTest2DTSDF (:30-47)
REF_TEST_OPTIONS = dict(truncation_distance=2.0, maximum_weight=10.0, update_free_space=False,
                        num_normal_samples=2, sample_radius=10.0,
                        project_sdf_distance_to_scan_normal=False, update_weight_range_exponent=0,
                        angle_kernel_bandwidth=0.0, distance_kernel_bandwidth=0.0)
REF_TEST_GRID = (1.0, (1.0, 7.0), 8, 1, 2.0, 10.0)     # TSDF2D(MapLimits(1, (1, 7), (8, 1)), 2, 10)
# configuration_files/trajectory_builder_2d.lua:100-112
LUA_DEFAULTS = dict(truncation_distance=0.3, maximum_weight=10.0, update_free_space=False,
                    num_normal_samples=4, sample_radius=0.5,
                    project_sdf_distance_to_scan_normal=True, update_weight_range_exponent=0,
                    angle_kernel_bandwidth=0.5, distance_kernel_bandwidth=0.5)

ONE_POINT = np.array([[-0.5, 3.5, 0.0]], np.float32)                       # InsertPoint (:50-56)
ORIGIN = np.array([-0.5, -0.5, 0.0], np.float32)


def options_vector(opts):
    return np.array([float(opts[k]) for k in OPTION_KEYS], np.float64)


def options_dict(vec):
    d = {k: float(v) for k, v in zip(OPTION_KEYS, vec)}
    for k in ("update_free_space", "project_sdf_distance_to_scan_normal"):
        d[k] = bool(d[k])
    for k in ("num_normal_samples", "update_weight_range_exponent"):
        d[k] = int(d[k])
    return d


def _ref_scenarios():
    o = REF_TEST_OPTIONS
    three = np.array([[-0.5, 3.5, 0], [5.5, 3.5, 0], [10.5, 3.5, 0]], np.float32)
    two = three[:2].copy()
    return {
        # InsertPoint + 1000 more (:96-149); the free-space variant (:151-203)
        "ref_insert_point": [(ORIGIN, ONE_POINT, o, 1), (ORIGIN, ONE_POINT, o, 1000)],
        "ref_free_space": [(ORIGIN, ONE_POINT, dict(o, update_free_space=True), 1),
                           (ORIGIN, ONE_POINT, dict(o, update_free_space=True), 1000)],
        "ref_linear_weight": [(ORIGIN, ONE_POINT, dict(o, update_weight_range_exponent=1), 1)],
        "ref_quadratic_weight": [(ORIGIN, ONE_POINT, dict(o, update_weight_range_exponent=2), 1)],
        "ref_small_angle": [(ORIGIN, three, o, 1)],                                  # :240-263
        "ref_normal_projection": [(ORIGIN, two, dict(o, project_sdf_distance_to_scan_normal=True),
                                   1)],                                              # :265-291
        "ref_angle_kernel": [(ORIGIN, two, dict(o, angle_kernel_bandwidth=10.0), 1)],   # :293-325
        "ref_distance_kernel": [(ORIGIN, ONE_POINT, dict(o, distance_kernel_bandwidth=10.0),
                                 1)],                                                # :327-345
    }


def room_scans(num_scans=12, beams=1000):
    """(origin, returns in the map frame) of `num_scans` scans of a seeded synthetic room."""
    from cartographer_amd import synth
    _, lim, world = synth.make_submap(17, 160, 160, 0.05, 4, 200, 6.0, 0.01)
    out = []
    for k in range(num_scans):
        at = world.free_pose(40 + k, 0.4)
        pts = world.scan(at, beams, 6.0, 0.01, 100 + k).astype(np.float64)
        c, s = np.cos(at[2]), np.sin(at[2])
        in_map = np.zeros((pts.shape[0], 3), np.float32)
        in_map[:, 0] = at[0] + c * pts[:, 0] - s * pts[:, 1]
        in_map[:, 1] = at[1] + s * pts[:, 0] + c * pts[:, 1]
        out.append((np.array([at[0], at[1], 0.0], np.float32), in_map))
    return out, lim


def _room_scenarios():
    scans, lim = room_scans()
    centre = (scans[0][0][0] + 0.4, scans[0][0][1] + 0.4)          # 16x16 cells of 5 cm
    grid = (0.05, centre, 16, 16, 0.3, 10.0)
    sets = {"room_lua": LUA_DEFAULTS,
            "room_free_space": dict(LUA_DEFAULTS, update_free_space=True),
            # no normals: the hits keep their input order
            "room_no_kernels": dict(LUA_DEFAULTS, project_sdf_distance_to_scan_normal=False,
                                    angle_kernel_bandwidth=0.0, distance_kernel_bandwidth=0.0)}
    return {name: (grid, [(o, r, opts, 1) for o, r in scans]) for name, opts in sets.items()}


def _edge_steps():
    rng = np.random.default_rng(7)
    origin = np.array([0.1, -0.2, 0.0], np.float32)
    steps = []
    # (a) dense beams: 400 hits on a 1 m wall 2 m ahead, free space on: the rays share cells
    y = np.linspace(-0.5, 0.5, 400)
    wall = np.stack([np.full_like(y, 2.1), y - 0.2, np.zeros_like(y)], 1).astype(np.float32)
    steps.append((origin, wall, dict(LUA_DEFAULTS, update_free_space=True), 1))
    # (b) duplicate points: 60 hits, each three times, shuffled
    ang = rng.uniform(-2.5, 2.5, 60)
    pts = np.stack([origin[0] + 1.5 * np.cos(ang), origin[1] + 1.5 * np.sin(ang),
                    np.zeros(60)], 1).astype(np.float32)
    dup = np.concatenate([pts, pts, pts])[rng.permutation(180)]
    steps.append((origin, dup, LUA_DEFAULTS, 1))
    # (c) hits closer than the truncation distance: skipped, but sorted and feeding the normals
    ang = np.linspace(-1.0, 1.0, 120)
    rad = np.where(np.arange(120) % 3 == 0, 0.15, 1.2)
    pts = np.stack([origin[0] + rad * np.cos(ang), origin[1] + rad * np.sin(ang),
                    np.zeros(120)], 1).astype(np.float32)
    steps.append((origin, pts, LUA_DEFAULTS, 1))
    # (d) a narrow angle kernel on a slanted wall: far from the normal the weight underflows to
    # 0 (UpdateCell returns unmarked) and a later ray takes the cell
    t = np.linspace(0.0, 1.0, 300)
    slanted = np.stack([origin[0] - 1.6 + 0.8 * t, origin[1] + 0.4 + 1.6 * t,
                        np.zeros(300)], 1).astype(np.float32)
    steps.append((origin, slanted[rng.permutation(300)],
                  dict(LUA_DEFAULTS, update_free_space=True, angle_kernel_bandwidth=0.01), 1))
    # (e) an empty insert whose origin lies outside the grid: GrowAsNeeded still grows it
    steps.append((np.array([4.5, 3.0, 0.0], np.float32), np.zeros((0, 3), np.float32),
                  LUA_DEFAULTS, 1))
    return steps


def scenarios():
    """{name: (grid args of ReferenceTSDF2D, [(origin, returns, options, repeat), ...])}."""
    out = {name: (REF_TEST_GRID, steps) for name, steps in _ref_scenarios().items()}
    out.update(_room_scenarios())
    out["edges"] = ((0.05, (3.2, 3.2), 128, 128, 0.3, 10.0), _edge_steps())
    return out


def digest(tsd, weight):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(tsd, np.uint16).tobytes() +
                                        np.ascontiguousarray(weight, np.uint16).tobytes()).digest(),
                         np.uint8)


def step_inputs(golden, name, k):
    """(origin, returns, options dict, repeat) of step k of scenario `name` in the .npz."""
    key = f"{name}/{k}"
    src = str(golden[key + "/returns_of"]) if key + "/returns_of" in golden else key
    return (golden[src + "/origin"], golden[src + "/returns"],
            options_dict(golden[key + "/options"]), int(golden[key + "/repeat"]))


def build():
    from oracle import pyoracle as orc
    if orc.ref_lib() is None:
        raise SystemExit("oracle/_ref is not built and /root/reference is absent")
    result = {}
    for name, (grid_args, steps) in scenarios().items():
        res, max_xy, nx, ny, truncation, max_weight = grid_args
        result[f"{name}/meta"] = np.array([res, max_xy[0], max_xy[1], nx, ny, truncation,
                                           max_weight], np.float64)
        grid = orc.ReferenceTSDF2D(res, max_xy, nx, ny, truncation, max_weight)
        for k, (origin, returns, opts, repeat) in enumerate(steps):
            for _ in range(repeat):
                grid.insert(origin, returns, **opts)
            tsd, wgt = grid.planes()
            lim = grid.limits
            key = f"{name}/{k}"
            if name.startswith("room_") and name != "room_lua":
                result[key + "/returns_of"] = np.array(f"room_lua/{k}")
            else:
                result[key + "/origin"] = np.asarray(origin, np.float32)
                result[key + "/returns"] = np.asarray(returns, np.float32).reshape(-1, 3)
            result[key + "/options"] = options_vector(opts)
            result[key + "/repeat"] = np.array(repeat, np.int32)
            result[key + "/digest"] = digest(tsd, wgt)
            if not name.startswith("room_") or k == len(steps) - 1:
                result[key + "/tsd"] = tsd
                result[key + "/weight"] = wgt
            result[key + "/limits"] = np.array([lim["resolution"], lim["max_x"], lim["max_y"],
                                                lim["num_x_cells"], lim["num_y_cells"]],
                                               np.float64)
    return result


if __name__ == "__main__":
    out = os.path.join(HERE, "tsdf_insert_golden.npz")
    np.savez_compressed(out, **build())
    print("wrote", out, os.path.getsize(out), "bytes")
