#!/usr/bin/env python3
"""Generates tests/golden/ceres2d_tsdf_golden.npz: residuals, Jacobians and solves of the
REFERENCE'S OWN TSDFMatchCostFunction2D and CeresScanMatcher2D::Match on a TSDF2D
(tsdf_match_cost_function_2d.cc, interpolated_tsdf_2d.h, ceres_scan_matcher_2d.cc compiled into
oracle/_ref/libref_ceres.so over the stand-in solver of oracle/ref_shims/ceres), for
tests/test_gpu_ceres_tsdf.py.  tests/native/ceres2d_tsdf_ref.cc is the driver; it is compiled into
a temporary directory.  The GPU box needs neither the reference nor the oracle.

Grids ("grid/<name>/..."):
  ref_fixture   TSDFSpaceCostFunction2DTest's grid (tsdf_match_cost_function_2d_test.cc:36-71):
                40x40 cells of 0.1 m, filled by the reference's own TSDFRangeDataInserter2D
  interp_points InterpolatedTSDF2DTest.InterpolatesGridPoints' grid (interpolated_tsdf_2d_test.cc:
                50-73), SetCell without FinishUpdate: every known tsd cell keeps the update marker
  interp_cell   InterpolatedTSDF2DTest.InterpolatesWithinCell's four cells (:96-111)
  room, room_marked, patch
                derived from the planes "room_lua/11/{tsd,weight}" of tsdf_insert_golden.npz (not
                copied): as they are; with bit 15 set on every third known cell of both planes;
                with every cell outside a 10x10 box cleared (a small known patch)
Residual cases ("res/<case>/..."): grid, scaling, poses [P, 3], xyz [P, m, 3], valid [P],
residuals [P, m], jacobian [P, m, 3] (zero where not valid).
Solves ("solve/<case>/..."): grid, options (occupied_space_weight, translation_weight,
rotation_weight, use_nonmonotonic_steps, max_num_iterations), target [2], init [3], the cloud
("xyz", or "xyz_of": a key of tsdf_insert_golden.npz), pose [3], summary (initial cost, final
cost, successful steps, unsuccessful steps, termination).  Usage:
    python tests/golden/make_ceres2d_tsdf_golden.py
"""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

INSERT_GOLDEN = os.path.join(HERE, "tsdf_insert_golden.npz")
ROOM = "room_lua/11"
MARKER = np.uint16(1 << 15)
# Plane rows and columns of the patch: a 10x10 block of the room whose cells are all known.
PATCH = (101, 111, 104, 114)

# configuration_files/trajectory_builder_2d.lua:48-56 (ceres_scan_matcher)
LOCAL_OPTIONS = (1.0, 10.0, 40.0, 0.0, 20.0)
# configuration_files/pose_graph.lua:42-50 (constraint_builder.ceres_scan_matcher)
CONSTRAINT_OPTIONS = (20.0, 10.0, 1.0, 1.0, 10.0)
LONG_OPTIONS = (20.0, 10.0, 1.0, 1.0, 50.0)


def room_grid(insert_golden, variant):
    """(tsd, weight, resolution, max_x, max_y, truncation, max_weight) of a room variant."""
    tsd = insert_golden[ROOM + "/tsd"].copy()
    wgt = insert_golden[ROOM + "/weight"].copy()
    lim = insert_golden[ROOM + "/limits"]
    meta = insert_golden["room_lua/meta"]
    if variant == "room_marked":
        known = np.flatnonzero(tsd.reshape(-1) != 0)
        every_third = known[known % 3 == 0]
        tsd.reshape(-1)[every_third] |= MARKER
        wgt.reshape(-1)[every_third] |= MARKER
    elif variant == "patch":
        keep = np.zeros(tsd.shape, bool)
        keep[PATCH[0]:PATCH[1], PATCH[2]:PATCH[3]] = True
        tsd[~keep] = 0
        wgt[~keep] = 0
    else:
        assert variant == "room", variant
    return tsd, wgt, float(lim[0]), float(lim[1]), float(lim[2]), float(meta[5]), float(meta[6])


def grid_of(golden, insert_golden, name):
    if name.startswith("room") or name == "patch":
        return room_grid(insert_golden, name)
    m = golden[f"grid/{name}/meta"]
    return (golden[f"grid/{name}/tsd"], golden[f"grid/{name}/weight"], float(m[0]), float(m[1]),
            float(m[2]), float(m[3]), float(m[4]))


def cloud_of(golden, insert_golden, key):
    if key + "/xyz_of" in golden:
        return insert_golden[str(golden[key + "/xyz_of"])]
    return golden[key + "/xyz"]


# ---------------------------------------------------------------- reference side ---
def _driver():
    from oracle import pyoracle as orc
    if not orc.build_ref_ceres():
        raise SystemExit("oracle/_ref/libref_ceres.so is not built and the reference is absent")
    ref_dir = os.path.join(ROOT, "oracle", "_ref")
    tmp = tempfile.mkdtemp(prefix="ceres2d_tsdf_")
    so = os.path.join(tmp, "libceres2d_tsdf_ref.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-DNDEBUG", "-ffp-contract=off", "-shared",
                           "-fPIC", "-I", os.path.join(ROOT, "oracle", "ref_shims"),
                           "-I", "/root/reference",
                           os.path.join(ROOT, "tests", "native", "ceres2d_tsdf_ref.cc"),
                           os.path.join(ref_dir, "libref_ceres.so"),
                           "-Wl,-rpath," + ref_dir, "-o", so])
    L = C.CDLL(so)
    u16, f32, f64 = (np.ctypeslib.ndpointer(t, flags="C_CONTIGUOUS")
                     for t in (np.uint16, np.float32, np.float64))
    grid_args = [u16, u16, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_float,
                 C.c_float]
    L.drv_tsdf_residuals.argtypes = grid_args + [C.c_double, f64, f32, C.c_int, f64, f64]
    L.drv_tsdf_residuals.restype = C.c_int
    L.drv_tsdf_match.argtypes = grid_args + [f64, f64, f64, f32, C.c_int, f64, f64]
    L.drv_tsdf_match.restype = None
    return L


def _grid_call_args(grid):
    tsd, wgt, res, mx, my, trunc, maxw = grid
    tsd = np.ascontiguousarray(tsd, np.uint16)
    wgt = np.ascontiguousarray(wgt, np.uint16)
    return [tsd, wgt, tsd.shape[1], tsd.shape[0], res, mx, my, trunc, maxw]


def ref_residuals(L, grid, scaling, poses, clouds):
    P, m = clouds.shape[0], clouds.shape[1]
    valid = np.zeros(P, np.int32)
    r = np.zeros((P, m), np.float64)
    J = np.zeros((P, m, 3), np.float64)
    args = _grid_call_args(grid)
    for p in range(P):
        rr, jj = np.zeros(max(m, 1)), np.zeros(max(3 * m, 1))
        cloud = np.ascontiguousarray(clouds[p], np.float32).reshape(-1, 3)
        valid[p] = L.drv_tsdf_residuals(*args, scaling, np.ascontiguousarray(poses[p], np.float64),
                                        cloud if m else np.zeros((1, 3), np.float32), m, rr, jj)
        if valid[p]:
            r[p] = rr[:m]
            J[p] = jj[:3 * m].reshape(m, 3)
    return valid, r, J


def ref_match(L, grid, options, target, init, xyz):
    pose, summary = np.zeros(3), np.zeros(5)
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    L.drv_tsdf_match(*_grid_call_args(grid), np.asarray(options, np.float64),
                     np.asarray(target, np.float64), np.asarray(init, np.float64),
                     xyz if xyz.shape[0] else np.zeros((1, 3), np.float32), xyz.shape[0], pose,
                     summary)
    return pose, summary


# ------------------------------------------------------------------------- grids ---
def _ref_fixture_grid():
    """TSDFSpaceCostFunction2DTest: TSDF2D(MapLimits(0.1, (2.05, 2.05), (40, 40)), 0.3, 1.0) and
    InsertPointcloud() (x from -0.5 while x < 0.5f, x += 0.1 in float), then FinishUpdate."""
    from oracle import pyoracle as orc
    grid = orc.ReferenceTSDF2D(0.1, (2.05, 2.05), 40, 40, 0.3, 1.0)
    xs, x = [], np.float32(-0.5)
    while x < np.float32(0.5):
        xs.append(x)
        x = np.float32(np.float64(x) + 0.1)
    returns = np.array([[v, 1.0, 0.0] for v in xs], np.float32)
    grid.insert(np.array([-0.5, -0.5, 0.0], np.float32), returns, truncation_distance=0.3,
                maximum_weight=1.0, update_free_space=False, num_normal_samples=2,
                sample_radius=10.0, project_sdf_distance_to_scan_normal=True,
                update_weight_range_exponent=0, angle_kernel_bandwidth=0.0,
                distance_kernel_bandwidth=0.0)
    tsd, wgt = grid.planes()
    lim = grid.limits
    tsd = tsd & np.uint16(0x7fff)            # FinishUpdate
    return tsd, wgt, lim["resolution"], lim["max_x"], lim["max_y"], 0.3, 1.0


def _set_cells(res, max_xy, n, truncation, max_weight, cells):
    """TSDF2D::SetCell (tsdf_2d.cc:58-71) for (x, y, tsd, weight) tuples, no FinishUpdate."""
    from oracle import pyoracle as orc
    L = orc.ref_lib()
    tsd = np.zeros((n, n), np.uint16)
    wgt = np.zeros((n, n), np.uint16)
    for x, y, t, w in cells:
        ix, iy = orc.ref_map_limits_cell_index(res, max_xy[0], max_xy[1], [[x, y]])[0]
        if tsd[iy, ix] & MARKER:
            continue
        tsd[iy, ix] = L.ref_tsd_float_to_value(0, truncation, max_weight, t) + int(MARKER)
        wgt[iy, ix] = L.ref_tsd_float_to_value(1, truncation, max_weight, w)
    return tsd, wgt, res, max_xy[0], max_xy[1], truncation, max_weight


def _interp_points_grid():
    cells = [(x, y, 0.1, 1.0) for x, y in ((1, 1), (2, 1), (1, 2), (2, 2))]
    for x in range(4):
        cells += [(x, 0, 0.1, 1.0), (x, 3, 0.1, 1.0)]
    for y in (1, 2):
        cells += [(0, y, 0.1, 1.0), (3, y, 0.1, 1.0)]
    return _set_cells(1.0, (5.5, 5.5), 10, 1.0, 10.0, cells)


def _interp_cell_grid():
    cells = [(0, 0, 0.1, 1.0), (0, 1, 0.2, 2.0), (1, 0, 0.3, 3.0), (1, 1, 0.4, 4.0)]
    return _set_cells(1.0, (5.5, 5.5), 10, 1.0, 10.0, cells)


# --------------------------------------------------------------------- scenarios ---
def _sweep(grid, rng, num_poses, m=6):
    """Poses and per-pose clouds whose world points hit cell centres, cell boundaries, the
    known/unknown border, random known cells and the outside; ~5% of the poses see no weight."""
    tsd, wgt, res, mx, my, _, _ = grid
    ny, nx = tsd.shape
    # Plane row iy = cell_index[1] runs with x, column ix = cell_index[0] with y (MapLimits'
    # flipped convention): the centre of [iy, ix] is (max_x - res (iy + .5), max_y - res (ix + .5)).
    known = np.argwhere((wgt & np.uint16(0x7fff)) != 0)                       # (iy, ix)
    unknown = (wgt & np.uint16(0x7fff)) == 0
    border = np.array([(iy, ix) for iy, ix in known
                       if 0 < iy < ny - 1 and 0 < ix < nx - 1 and
                       (unknown[iy - 1, ix] or unknown[iy + 1, ix] or unknown[iy, ix - 1] or
                        unknown[iy, ix + 1])])
    f32 = np.float32
    poses = np.zeros((num_poses, 3))
    clouds = np.zeros((num_poses, m, 3), np.float32)
    for p in range(num_poses):
        kind = p % 10
        if kind < 3:
            pose = np.zeros(3)                                     # world == cloud, exactly
        elif kind < 7:
            pose = np.array([rng.integers(-8, 9) * res / 4, rng.integers(-8, 9) * res / 4, 0.0])
        else:
            pose = np.array([rng.uniform(-0.2, 0.2), rng.uniform(-0.2, 0.2),
                             rng.uniform(-0.3, 0.3)])
        world = np.zeros((m, 2))
        for i in range(m):
            what = rng.integers(0, 6) if p % 20 != 19 else 6
            iy, ix = known[rng.integers(len(known))]
            if what == 0:                                          # a cell centre
                world[i] = [f32(mx - res * (iy + 0.5)), f32(my - res * (ix + 0.5))]
            elif what == 1:                                        # a cell boundary / corner
                world[i] = [f32(mx - res * iy), f32(my - res * (ix + rng.integers(0, 2) * 0.5))]
            elif what == 2:                                        # the known/unknown border
                by, bx = border[rng.integers(len(border))]
                world[i] = [f32(mx - res * (by + rng.choice([0.0, 0.5, 1.0]))),
                            f32(my - res * (bx + rng.choice([0.0, 0.5, 1.0])))]
            elif what == 3:                                        # anywhere in a known cell
                world[i] = [mx - res * (iy + rng.uniform()), my - res * (ix + rng.uniform())]
            elif what == 4:                                        # outside the grid
                beyond = 0.3 * rng.uniform() + 0.01
                world[i] = [mx + beyond if rng.uniform() < 0.5 else mx - ny * res - beyond,
                            my - rng.uniform(-0.5, nx * res + 0.5)]
            elif what == 5:                                        # anywhere near the grid
                world[i] = [mx - rng.uniform(-0.2, ny * res + 0.2),
                            my - rng.uniform(-0.2, nx * res + 0.2)]
            else:                                                  # far away: S == 0
                world[i] = [mx + 5.0 + rng.uniform(), my + 5.0 + rng.uniform()]
        c, s = np.cos(pose[2]), np.sin(pose[2])
        d = world - pose[:2]
        clouds[p, :, 0] = c * d[:, 0] + s * d[:, 1]
        clouds[p, :, 1] = -s * d[:, 0] + c * d[:, 1]
        poses[p] = pose
    return poses, clouds


def scenarios(insert_golden):
    """(grids {name: grid}, residual cases, solve cases) without the reference's results."""
    grids = {"ref_fixture": _ref_fixture_grid(), "interp_points": _interp_points_grid(),
             "interp_cell": _interp_cell_grid()}
    for name in ("room", "room_marked", "patch"):
        grids[name] = room_grid(insert_golden, name)
    res = {}
    one = lambda x, y: np.array([[[x, y, 0.0]]], np.float32)            # noqa: E731
    zero_pose = np.zeros((1, 3))
    # tsdf_match_cost_function_2d_test.cc: MatchEmptyTSDF (an unfilled grid of the same limits)
    empty = tuple([np.zeros((40, 40), np.uint16), np.zeros((40, 40), np.uint16)] +
                  list(grids["ref_fixture"][2:]))
    grids["ref_empty"] = empty
    res["match_empty_tsdf"] = ("ref_empty", 1.0, zero_pose, one(0.0, 0.0))
    res["exact_initial_pose"] = ("ref_fixture", 1.0, zero_pose, one(0.0, 1.0))
    res["perturbated_initial_pose"] = ("ref_fixture", 1.0, np.array([[0, 0.1, 0], [0, -0.1, 0]]),
                                       np.repeat(one(0.0, 1.0), 2, 0))
    res["invalid_initial_pose"] = ("ref_fixture", 1.0, np.array([[0, 0.4, 0], [0, -0.4, 0]]),
                                   np.repeat(one(0.0, 1.0), 2, 0))
    # interpolated_tsdf_2d_test.cc as one-point clouds (the residual is then n s C = C)
    pts = [(1, 1), (2, 1), (1, 2), (2, 2), (3, 2)]
    res["interpolates_grid_points"] = ("interp_points", 1.0, np.zeros((len(pts), 3)),
                                       np.array([[[x, y, 0]] for x, y in pts], np.float32))
    inner = [(x, y) for x in (0.01, 0.25, 0.5, 0.77, 0.99) for y in (0.01, 0.3, 0.5, 0.9)]
    res["interpolates_within_cell"] = ("interp_cell", 1.0, np.zeros((len(inner), 3)),
                                       np.array([[[x, y, 0]] for x, y in inner], np.float32))
    rng = np.random.default_rng(2024)
    for name in ("room", "room_marked"):
        poses, clouds = _sweep(grids[name], rng, 1000)
        res[f"sweep_{name}"] = (name, 0.7, poses, clouds)
    # an empty cloud: what the reference does with n == 0
    res["empty_cloud"] = ("room", 1.0, zero_pose, np.zeros((1, 0, 3), np.float32))

    solves = {}
    for opt_name, opts in (("local", LOCAL_OPTIONS), ("constraint", CONSTRAINT_OPTIONS),
                           ("long", LONG_OPTIONS)):
        for k in range(8):
            scan = k + (0 if opt_name == "local" else 4 if opt_name == "constraint" else 2)
            init = np.array([rng.uniform(-0.06, 0.06), rng.uniform(-0.06, 0.06),
                             rng.uniform(-0.06, 0.06)])
            target = init[:2] + (rng.uniform(-0.02, 0.02, 2) if k % 2 else 0.0)
            solves[f"{opt_name}_{k}"] = ("room" if k != 7 else "room_marked", opts, target, init,
                                        f"room_lua/{scan % 12}/returns")
    # the initial pose in unknown space: FAILURE
    solves["failure"] = ("room", LOCAL_OPTIONS, np.array([40.0, 40.0]),
                         np.array([40.0, 40.0, 0.1]), "room_lua/0/returns")
    # a target that pulls the scan off a small known patch: candidate evaluations fail
    tsd, wgt, r, mx, my, _, _ = grids["patch"]
    pts = np.concatenate([insert_golden[f"room_lua/{k}/returns"] for k in range(12)])
    iy = np.round((mx - pts[:, 0].astype(np.float64)) / r - 0.5).astype(int)
    ix = np.round((my - pts[:, 1].astype(np.float64)) / r - 0.5).astype(int)
    keep = ((iy >= PATCH[0] + 2) & (iy < PATCH[1] - 2) & (ix >= PATCH[2] + 2) &
            (ix < PATCH[3] - 2))
    patch_cloud = pts[keep][::2].copy()           # the returns well inside the patch
    for k, (shift, opts) in enumerate(((3.0, LOCAL_OPTIONS), (1.0, CONSTRAINT_OPTIONS),
                                       (0.5, LONG_OPTIONS))):
        solves[f"patch_{k}"] = ("patch", opts, np.array([shift, -shift]),
                                np.array([0.005, -0.005, 0.002]), patch_cloud)
    solves["empty_cloud"] = ("room", LOCAL_OPTIONS, np.zeros(2), np.zeros(3),
                             np.zeros((0, 3), np.float32))
    return grids, res, solves


def build():
    insert_golden = np.load(INSERT_GOLDEN)
    L = _driver()
    grids, res, solves = scenarios(insert_golden)
    out = {}
    for name, g in grids.items():
        if name.startswith("room") or name == "patch":
            continue
        out[f"grid/{name}/tsd"] = np.asarray(g[0], np.uint16)
        out[f"grid/{name}/weight"] = np.asarray(g[1], np.uint16)
        out[f"grid/{name}/meta"] = np.array(g[2:], np.float64)
    for case, (grid, scaling, poses, clouds) in res.items():
        valid, r, J = ref_residuals(L, grids[grid], scaling, poses, clouds)
        key = f"res/{case}"
        out[key + "/grid"] = np.array(grid)
        out[key + "/scaling"] = np.array(scaling)
        out[key + "/poses"] = np.asarray(poses, np.float64)
        out[key + "/xyz"] = np.asarray(clouds, np.float32)
        out[key + "/valid"] = valid
        out[key + "/residuals"] = r
        out[key + "/jacobian"] = J
    for case, (grid, opts, target, init, cloud) in solves.items():
        key = f"solve/{case}"
        if isinstance(cloud, str):
            xyz = insert_golden[cloud]
            out[key + "/xyz_of"] = np.array(cloud)
        else:
            xyz = cloud
            out[key + "/xyz"] = np.asarray(cloud, np.float32)
        pose, summary = ref_match(L, grids[grid], opts, target, init, xyz)
        out[key + "/grid"] = np.array(grid)
        out[key + "/options"] = np.asarray(opts, np.float64)
        out[key + "/target"] = np.asarray(target, np.float64)
        out[key + "/init"] = np.asarray(init, np.float64)
        out[key + "/pose"] = pose
        out[key + "/summary"] = summary
    return out


if __name__ == "__main__":
    path = os.path.join(HERE, "ceres2d_tsdf_golden.npz")
    np.savez_compressed(path, **build())
    print("wrote", path, os.path.getsize(path), "bytes")
