"""Edge cases of the two Ceres refinement kernels (Ceres2DKernel<false> in csrc/ceres_2d.hip, the
3D kernel in csrc/ceres_3d.hip): single Levenberg-Marquardt steps, grid borders, step control and
cloud sizes.  Shared by tests/test_ceres_edge_cases.py (the table on the oracle alone: every case
reaches the branch it is named for and is stable under the device's legitimate differences) and
tests/test_gpu_ceres_edges.py (device against oracle).  Everything is regenerated from seeds; the
scenes are built once per process and handed out read-only.

Families:
  one_step  max_num_iterations = 1 from a pose 5 - 10 cm and 0.05 rad off: after one iteration the
            pose is a closed function of cost, J^T r and J^T J at the initial pose
  border    the cloud crosses an edge / face of the grid, a corner, or lies wholly outside
  step      rejected steps, non-monotonic acceptance, the iteration cap
  size      clouds from one point to 4097 (wavefront 64, workgroup 256 and their neighbours)

2D geometry (cells[iy][ix], ny rows by nx columns): iy counts down from max_x and ix down from
max_y, so the map covers x in [max_x - ny res, max_x] and y in [max_y - nx res, max_y].  The
bicubic stencil of a point is the 4 x 4 cells around it; outside the grid it reads the padding
constant.  3D: the device gathers the eight voxels around a point from the dense bounding box of
the voxel list; beyond a face of that box it reads value 0 (kMinProbability).
"""
import functools
import math
from dataclasses import dataclass, field

import numpy as np

from test_oracle_reference_pins_3d import quat_from_angle_axis

RES_2D = 0.05
NX_2D, NY_2D = 96, 150
SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 4097)
TERMINATION_CONVERGENCE, TERMINATION_NO_CONVERGENCE = 0, 1

# The names of the cases, for parametrising without building a scene (cases_2d / cases_3d check
# that they build exactly these).
NAMES_2D = (
    "one_step_monotonic", "one_step_nonmonotonic",
    "border_plus_x", "border_minus_x", "border_plus_y", "border_minus_y",
    "border_corner_minus_x_minus_y", "border_corner_minus_x_plus_y",
    "border_all_outside_target_off", "border_all_outside_zero_gradient",
    "step_rejected_a_monotonic", "step_rejected_a_nonmonotonic", "step_rejected_b_monotonic",
    "step_rejected_b_nonmonotonic", "step_cap_1", "step_cap_2", "step_cap_3",
) + tuple("size_%d" % n for n in SIZES)
NAMES_3D = (
    "one_step_quaternion_1_pairs", "one_step_quaternion_2_pairs", "one_step_quaternion_3_pairs",
    "one_step_yaw_1_pairs", "one_step_yaw_2_pairs", "one_step_yaw_3_pairs",
    "one_step_intensity_huber_0.3", "one_step_intensity_huber_1e+06",
    "border_plus_x", "border_minus_x", "border_plus_y", "border_minus_y", "border_plus_z",
    "border_minus_z", "border_all_outside", "border_negative_indices",
    "step_weak_a_monotonic", "step_weak_a_nonmonotonic", "step_weak_b_monotonic",
    "step_weak_b_nonmonotonic", "step_cap_3",
) + tuple("size_%d" % n for n in SIZES) + ("size_1_and_1000", "size_1000_and_1")


def _frozen(a):
    """A read-only copy: a prefix of a scan must not share its address with the scan (the batch
    entries tell clouds apart by address)."""
    a = np.array(a, order="C", copy=True)
    a.setflags(write=False)
    return a


# ================================================================================ 2D ============
@dataclass
class Case2D:
    name: str
    family: str
    cloud: np.ndarray
    init: tuple                    # initial pose estimate (x, y, theta)
    target: tuple                  # target translation (x, y)
    weights: tuple = (1.0, 10.0, 40.0)          # occupied space, translation, rotation
    nonmonotonic: bool = False
    iterations: int = 20
    # what the oracle must report for the case to be worth running
    termination: int = None
    min_successful: int = 0
    min_unsuccessful: int = 0
    steps: tuple = None            # exact (successful, unsuccessful)
    min_outside: int = 0           # points whose whole stencil lies outside the grid
    min_straddling: dict = field(default_factory=dict)   # edge -> stencils across it


@dataclass
class Scene2D:
    cells: np.ndarray
    lim: dict
    truth: np.ndarray
    scan: np.ndarray               # 300 beams
    dense: np.ndarray              # 6000 beams, for the 4097-point cloud


@functools.lru_cache(maxsize=None)
def scene_2d(synth):
    """The non-square submap (96 columns by 150 rows: 7.5 m in x, 4.8 m in y) and its scans."""
    cells, lim, world = synth.make_submap(31, NX_2D, NY_2D, RES_2D, 12, 400, 5.0, 0.01)
    truth = world.free_pose(36, 0.5)
    scan = world.scan(truth, 300, 5.0, 0.01, 4)
    dense = world.scan(truth, 6000, 5.0, 0.01, 5)
    assert scan.shape[0] >= 257 and dense.shape[0] >= 4097, (scan.shape, dense.shape)
    return Scene2D(_frozen(cells), lim, _frozen(truth), _frozen(scan), _frozen(dense))


def stencils_2d(lim, init, cloud):
    """Where the 4 x 4 stencils of `cloud` at pose `init` lie: (outside, straddling) with
    outside the number of points whose stencil has no cell in the grid and straddling =
    {"+x", "-x", "+y", "-y"} -> number of stencils with cells on both sides of that edge."""
    x, y, t = init
    c, s = math.cos(t), math.sin(t)
    pts = np.asarray(cloud, np.float64)
    wx = c * pts[:, 0] - s * pts[:, 1] + x
    wy = s * pts[:, 0] + c * pts[:, 1] + y
    row = np.floor((lim["max_x"] - wx) / lim["resolution"] - 0.5).astype(np.int64)   # iy
    col = np.floor((lim["max_y"] - wy) / lim["resolution"] - 0.5).astype(np.int64)   # ix
    ny, nx = lim["num_y_cells"], lim["num_x_cells"]
    r_lo, r_hi, c_lo, c_hi = row - 1, row + 2, col - 1, col + 2
    rows_in = (r_hi >= 0) & (r_lo < ny)
    cols_in = (c_hi >= 0) & (c_lo < nx)
    touches = rows_in & cols_in
    straddling = {"+x": int((touches & (r_lo < 0)).sum()),
                  "-x": int((touches & (r_hi >= ny)).sum()),
                  "+y": int((touches & (c_lo < 0)).sum()),
                  "-y": int((touches & (c_hi >= nx)).sum())}
    return int((~touches).sum()), straddling


# Shifts of the initial pose off the truth that carry the cloud across the named edges.
BORDER_SHIFTS_2D = (
    ("plus_x", (5.25, 0.0, 0.1), ("+x",)),
    ("minus_x", (-1.2, 0.0, 0.1), ("-x",)),
    ("plus_y", (0.0, 2.1, 0.1), ("+y",)),
    ("minus_y", (0.0, -0.9, 0.1), ("-y",)),
    ("corner_minus_x_minus_y", (-2.0, -1.0, 0.4), ("-x", "-y")),
    ("corner_minus_x_plus_y", (-2.0, 2.25, 0.8), ("-x", "+y")),
)


@functools.lru_cache(maxsize=None)
def cases_2d(synth):
    sc = scene_2d(synth)
    truth, scan = sc.truth, sc.scan
    out = []

    def at(dx, dy, dt):
        return (float(truth[0] + dx), float(truth[1] + dy), float(truth[2] + dt))

    # (a) one step
    near = at(0.07, -0.05, 0.05)
    near_target = (near[0] + 0.01, near[1] - 0.01)
    for nonmono in (False, True):
        out.append(Case2D("one_step_%s" % ("nonmonotonic" if nonmono else "monotonic"), "one_step",
                          scan, near, near_target, (20.0, 10.0, 1.0), nonmono, 1,
                          termination=TERMINATION_NO_CONVERGENCE, steps=(1, 0)))
    # (b) borders
    for name, shift, edges in BORDER_SHIFTS_2D:
        init = at(*shift)
        out.append(Case2D("border_" + name, "border", scan, init,
                          (init[0] - 0.02, init[1] + 0.01), (20.0, 10.0, 1.0), False, 10,
                          min_successful=1, min_outside=5,
                          min_straddling={e: 5 for e in edges}))
    far = at(20.0, -15.0, 0.3)
    out.append(Case2D("border_all_outside_target_off", "border", scan, far,
                      (far[0] + 0.03, far[1] - 0.02), (20.0, 10.0, 1.0), False, 10,
                      termination=TERMINATION_CONVERGENCE, min_successful=1,
                      min_outside=scan.shape[0]))
    out.append(Case2D("border_all_outside_zero_gradient", "border", scan, far, far[:2],
                      (20.0, 10.0, 1.0), False, 10, termination=TERMINATION_CONVERGENCE,
                      steps=(0, 0), min_outside=scan.shape[0]))
    # (d) step control: the weights of the one case of the suite that rejects a step
    wide = at(-0.28, 0.26, 0.11)
    for name, start in (("a", wide), ("b", at(0.37, -0.28, -0.01))):
        for nonmono in (False, True):
            out.append(Case2D("step_rejected_%s_%s" % (name, "nonmonotonic" if nonmono
                                                       else "monotonic"),
                              "step", scan, start, start[:2], (5.0, 1.0, 1.0), nonmono, 50,
                              min_successful=2, min_unsuccessful=1))
    for cap in (1, 2, 3):
        out.append(Case2D("step_cap_%d" % cap, "step", scan, wide, wide[:2], (5.0, 1.0, 1.0), True,
                          cap, termination=TERMINATION_NO_CONVERGENCE))
    # (e) cloud sizes: prefixes of one scan
    for n in SIZES:
        cloud = _frozen((sc.dense if n > scan.shape[0] else scan)[:n])
        out.append(Case2D("size_%d" % n, "size", cloud, near, near_target, (20.0, 10.0, 1.0),
                          False, 10, min_successful=1))
    assert tuple(c.name for c in out) == NAMES_2D
    return tuple(out)


def oracle_2d(orc, synth, case, cloud=None, init=None, reference=False):
    sc = scene_2d(synth)
    w = case.weights
    return orc.ceres2d_match(sc.cells, RES_2D, sc.lim["max_x"], sc.lim["max_y"], case.target,
                             case.init if init is None else init,
                             case.cloud if cloud is None else cloud, w[0], w[1], w[2],
                             case.nonmonotonic, case.iterations, reference=reference)


# ================================================================================ 3D ============
@dataclass
class Case3D:
    name: str
    family: str
    pairs: tuple                   # ((cloud, resolution, voxels[, intensities, ivoxels, opts]), ...)
    weights: tuple                 # occupied_space_weight per pair
    init_t: tuple
    yaw: float                     # the initial rotation is AngleAxis(yaw, axis)
    target: tuple
    axis: tuple = (0.05, -0.02, 1.0)
    translation_weight: float = 5.0
    rotation_weight: float = 4e2
    yaw_only: bool = False
    nonmonotonic: bool = False
    iterations: int = 12
    resident: bool = False         # also run through match_grids on the resident grids
    termination: int = None
    min_successful: int = 0
    min_unsuccessful: int = 0
    steps: tuple = None
    min_outside: int = 0           # points (first pair) whose eight voxels all lie outside the box
    min_straddling: dict = field(default_factory=dict)   # face -> gathers across it (first pair)

    @property
    def intensity(self):
        return any(len(p) > 3 for p in self.pairs)

    def init7(self, yaw=None):
        return list(self.init_t) + quat_from_angle_axis(self.yaw if yaw is None else yaw,
                                                        list(self.axis))

    def options(self):
        return dict(translation_weight=self.translation_weight,
                    rotation_weight=self.rotation_weight, only_optimize_yaw=self.yaw_only,
                    use_nonmonotonic_steps=self.nonmonotonic, max_num_iterations=self.iterations)


SCAN_YAW_3D = 0.4
INSERT_POSES_3D = 4
# whole voxels of the 0.1 m, 0.2 m and 0.3 m grids: 120, 60 and 40
NEGATIVE_OFFSET_M = -12.0


@dataclass
class Scene3D:
    pos: np.ndarray
    hi: np.ndarray
    lo: np.ndarray
    mid: np.ndarray
    dense: np.ndarray              # 40 rings, for the 4097-point cloud
    vox: np.ndarray                # 0.1 m grid
    low_vox: np.ndarray            # 0.3 m grid
    mid_vox: np.ndarray            # 0.2 m grid
    inserts: tuple                 # ((origin f32[3], returns in the map frame f32[n, 3]), ...)


def insert_scans_3d(synth, seed=7):
    """The scans make_submap_3d(seed, r, (8, 8, 4), 4, 8, 96) inserts, as (origin, returns)."""
    world = synth.World3D(seed, (8.0, 8.0, 4.0))
    out = []
    for p in range(INSERT_POSES_3D):
        pos = world.free_position(seed * 1009 + p, 0.5)
        yaw = 0.37 * p
        sensor = world.scan(pos, yaw, 8, 96, seed=seed * 31 + p).astype(np.float64)
        c, s = np.cos(yaw), np.sin(yaw)
        in_map = np.stack([pos[0] + c * sensor[:, 0] - s * sensor[:, 1],
                           pos[1] + s * sensor[:, 0] + c * sensor[:, 1],
                           pos[2] + sensor[:, 2]], 1).astype(np.float32)
        out.append((_frozen(pos.astype(np.float32)), _frozen(in_map)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def scene_3d(synth):
    grid, world = synth.make_submap_3d(7, 0.1, (8.0, 8.0, 4.0), 4, 8, 96)
    low, _ = synth.make_submap_3d(7, 0.3, (8.0, 8.0, 4.0), 4, 8, 96)
    mid, _ = synth.make_submap_3d(7, 0.2, (8.0, 8.0, 4.0), 4, 8, 96)
    pos = world.free_position(8, 0.5)
    full = world.scan(pos, SCAN_YAW_3D, 16, 128, seed=3)
    dense = world.scan(pos, SCAN_YAW_3D, 40, 128, seed=5)
    assert dense.shape[0] >= 4097, dense.shape
    return Scene3D(_frozen(pos), _frozen(full[::2]), _frozen(full[::9]), _frozen(full[1::5]),
                   _frozen(dense), _frozen(grid.voxels()), _frozen(low.voxels()),
                   _frozen(mid.voxels()), insert_scans_3d(synth))


def _to_world(init7, cloud):
    w, u = init7[3], np.asarray(init7[4:7], np.float64)
    v = np.asarray(cloud, np.float64)
    uv = 2.0 * np.cross(u, v)
    return v + w * uv + np.cross(u, uv) + np.asarray(init7[:3], np.float64)


def gathers_3d(resolution, voxels, init7, cloud):
    """Where the eight-voxel gathers of `cloud` at pose `init7` lie against the bounding box of
    `voxels`: (outside, straddling, corrected) with straddling = {"+x", "-x", ...} -> gathers with
    voxels on both sides of that face, corrected = lower voxels moved down by one (cx -= res)."""
    res = np.float32(resolution)
    p = _to_world(init7, cloud)
    at = np.rint(p.astype(np.float32) / res)
    centre = at.astype(np.float32) * res
    below = centre.astype(np.float64) > p
    centre = np.where(below, centre - res, centre).astype(np.float32)
    i1 = np.rint(centre / res).astype(np.int64)
    lo = np.array([voxels["x"].min(), voxels["y"].min(), voxels["z"].min()], np.int64)
    hi = np.array([voxels["x"].max(), voxels["y"].max(), voxels["z"].max()], np.int64)
    overlap = (i1 + 1 >= lo) & (i1 <= hi)
    touches = overlap.all(axis=1)
    straddling = {}
    for k, axis in enumerate("xyz"):
        straddling["-" + axis] = int((touches & (i1[:, k] < lo[k])).sum())
        straddling["+" + axis] = int((touches & (i1[:, k] + 1 > hi[k])).sum())
    return int((~touches).sum()), straddling, int(below.sum())


def shifted_voxels(voxels, resolution, offset_m):
    """The voxel list moved by offset_m along every axis (a whole number of voxels)."""
    steps = offset_m / resolution
    assert abs(steps - round(steps)) < 1e-9, (offset_m, resolution)
    out = voxels.copy()
    for axis in "xyz":
        out[axis] += int(round(steps))
    return _frozen(out)


# Shifts of the initial translation off the scan position that carry the cloud across the faces
# of the 0.1 m grid's box (voxels [-40, 40] x [-40, 40] x [0, 40]).
BORDER_SHIFTS_3D = (
    ("plus_x", (2.75, 0.0, 0.0), "+x"),
    ("minus_x", (-2.5, 0.0, 0.0), "-x"),
    ("plus_y", (0.0, 4.75, 0.0), "+y"),
    ("minus_y", (0.0, -2.0, 0.0), "-y"),
    ("plus_z", (0.0, 0.0, 2.0), "+z"),
    ("minus_z", (0.0, 0.0, -1.0), "-z"),
)


@functools.lru_cache(maxsize=None)
def cases_3d(synth, orc):
    from test_reference_ref_ceres import _intensity_world
    sc = scene_3d(synth)
    pos = np.asarray(sc.pos)
    hi_pair, lo_pair = (sc.hi, 0.1, sc.vox), (sc.lo, 0.3, sc.low_vox)
    mid_pair = (sc.mid, 0.2, sc.mid_vox)
    two, two_w = (hi_pair, lo_pair), (1.0, 6.0)
    out = []

    def at(d):
        return tuple(float(v) for v in pos + np.asarray(d))

    # (a) one step
    near = at((0.06, -0.05, 0.05))
    near_target = at((0.05, -0.04, 0.04))
    for yaw_only in (False, True):
        for pairs, weights in (((hi_pair,), (1.0,)), (two, two_w),
                               ((hi_pair, mid_pair, lo_pair), (1.0, 3.0, 6.0))):
            out.append(Case3D("one_step_%s_%d_pairs" % ("yaw" if yaw_only else "quaternion",
                                                        len(pairs)), "one_step", pairs, weights,
                              near, SCAN_YAW_3D + 0.05, near_target, yaw_only=yaw_only,
                              iterations=1, resident=True,
                              termination=TERMINATION_NO_CONVERGENCE, steps=(1, 0)))
    vox, iv, ipos, icloud, intensities = _intensity_world(synth, orc, 7)
    inear = tuple(float(v) for v in np.asarray(ipos) + np.array([0.06, -0.05, 0.05]))
    for huber_scale in (0.3, 1e6):
        pairs = ((_frozen(icloud), 0.1, _frozen(vox), _frozen(intensities), _frozen(iv),
                  (0.5, huber_scale, 100.0)), (_frozen(icloud[::4]), 0.3, sc.low_vox))
        out.append(Case3D("one_step_intensity_huber_%g" % huber_scale, "one_step", pairs, two_w,
                          inear, 0.3 + 0.05, inear, iterations=1,
                          termination=TERMINATION_NO_CONVERGENCE, steps=(1, 0)))
    # (c) borders
    for name, shift, face in BORDER_SHIFTS_3D:
        init_t = at(shift)
        out.append(Case3D("border_" + name, "border", two, two_w, init_t, SCAN_YAW_3D + 0.02,
                          init_t, iterations=12, resident=True, min_successful=1, min_outside=5,
                          min_straddling={face: 5}))
    far = at((30.0, -20.0, 10.0))
    out.append(Case3D("border_all_outside", "border", two, two_w, far, SCAN_YAW_3D + 0.02, far,
                      iterations=12, resident=True, termination=TERMINATION_CONVERGENCE,
                      steps=(0, 0), min_outside=sc.hi.shape[0]))
    moved = ((sc.hi, 0.1, shifted_voxels(sc.vox, 0.1, NEGATIVE_OFFSET_M)),
             (sc.lo, 0.3, shifted_voxels(sc.low_vox, 0.3, NEGATIVE_OFFSET_M)))
    assert max(moved[0][2][a].max() for a in "xyz") < 0
    moved_t = at((0.04 + NEGATIVE_OFFSET_M, -0.03 + NEGATIVE_OFFSET_M, 0.02 + NEGATIVE_OFFSET_M))
    out.append(Case3D("border_negative_indices", "border", moved, two_w, moved_t,
                      SCAN_YAW_3D + 0.02, moved_t, iterations=12, min_successful=1))
    # (d) step control: weak weights reject steps
    for name, tw, rw, offset, yaw_error in (("a", 0.01, 0.1, (0.15, -0.1, 0.05), 0.05),
                                            ("b", 5.0, 0.1, (0.4, 0.3, -0.2), 0.3)):
        init_t = at(offset)
        for nonmono in (False, True):
            out.append(Case3D("step_weak_%s_%s" % (name, "nonmonotonic" if nonmono else "monotonic"),
                              "step", two, two_w, init_t, SCAN_YAW_3D + yaw_error, init_t,
                              translation_weight=tw, rotation_weight=rw, nonmonotonic=nonmono,
                              iterations=40, min_successful=2, min_unsuccessful=1))
    out.append(Case3D("step_cap_3", "step", two, two_w, at((0.15, -0.1, 0.05)), SCAN_YAW_3D + 0.05,
                      at((0.15, -0.1, 0.05)), translation_weight=0.01, rotation_weight=0.1,
                      nonmonotonic=True, iterations=3, termination=TERMINATION_NO_CONVERGENCE))
    # (e) cloud sizes: one pair with prefixes of a wall-first ordering of the cloud, and a
    # one-point pair next to a thousand-point pair
    walls = wall_first(sc)
    for n in SIZES:
        cloud = _frozen((sc.dense if n > walls.shape[0] else walls)[:n])
        out.append(Case3D("size_%d" % n, "size", ((cloud, 0.1, sc.vox),), (1.0,), near,
                          SCAN_YAW_3D + 0.02, near_target, iterations=12, min_successful=1))
    thousand = _frozen(sc.hi[:1000])
    one_hi, one_lo = _frozen(walls[:1]), _frozen(walls[:1])
    out.append(Case3D("size_1_and_1000", "size", ((one_hi, 0.1, sc.vox), (thousand, 0.3, sc.low_vox)),
                      two_w, near, SCAN_YAW_3D + 0.02, near_target, min_successful=1))
    out.append(Case3D("size_1000_and_1", "size", ((thousand, 0.1, sc.vox), (one_lo, 0.3, sc.low_vox)),
                      two_w, near, SCAN_YAW_3D + 0.02, near_target, min_successful=1))
    assert tuple(c.name for c in out) == NAMES_3D
    return tuple(out)


def wall_first(sc):
    """The high-resolution cloud with the points that lie on a wall first: those whose nearest
    voxel at the true pose is occupied (value above one half), in scan order.  A prefix of the raw
    scan may begin in unknown space, where the cost is flat and the solve takes no step."""
    init7 = list(sc.pos) + quat_from_angle_axis(SCAN_YAW_3D, [0.0, 0.0, 1.0])
    p = _to_world(init7, sc.hi)
    at = np.rint(p.astype(np.float32) / np.float32(0.1)).astype(np.int64)
    occupied = {(int(v["x"]), int(v["y"]), int(v["z"])) for v in sc.vox
                if (int(v["value"]) & 0x7fff) > 16384}
    on_wall = np.array([tuple(i) in occupied for i in at])
    order = np.concatenate([np.flatnonzero(on_wall), np.flatnonzero(~on_wall)])
    return _frozen(np.asarray(sc.hi)[order])


def oracle_3d(orc, case, pairs=None, yaw=None, reference=False):
    pairs = list(case.pairs if pairs is None else pairs)
    fn = orc.ceres3d_match_intensity if case.intensity else orc.ceres3d_match
    return fn(pairs, case.target, case.init7(yaw), list(case.weights), reference=reference,
              **case.options())


# ================================================================== stability of a case ==========
PERMUTATIONS = 20


def ulp_neighbours(angle):
    return (float(np.nextafter(angle, -np.inf)), float(np.nextafter(angle, np.inf)))


def perturbed_2d(orc, synth, case):
    """The oracle's results on what the device may legitimately see differently: the cloud in
    PERMUTATIONS random orders (another order of the f64 sums) and the initial angle one ulp to
    either side (sin / cos that differ by about an ulp)."""
    rng = np.random.default_rng(len(case.name) + case.cloud.shape[0])
    out = []
    for _ in range(PERMUTATIONS):
        out.append(oracle_2d(orc, synth, case, cloud=case.cloud[rng.permutation(case.cloud.shape[0])]))
    for angle in ulp_neighbours(case.init[2]):
        out.append(oracle_2d(orc, synth, case, init=(case.init[0], case.init[1], angle)))
    return out


def perturbed_3d(orc, case):
    rng = np.random.default_rng(len(case.name) + case.pairs[0][0].shape[0])
    out = []
    for _ in range(PERMUTATIONS):
        pairs = []
        for p in case.pairs:
            order = rng.permutation(p[0].shape[0])
            q = (p[0][order],) + tuple(p[1:3])
            if len(p) > 3:
                q += (p[3][order],) + tuple(p[4:])
            pairs.append(q)
        out.append(oracle_3d(orc, case, pairs=pairs))
    for angle in ulp_neighbours(case.yaw):
        out.append(oracle_3d(orc, case, yaw=angle))
    return out


def counts(result):
    return (result["num_successful_steps"], result["num_unsuccessful_steps"], result["termination"])


# The one-step tolerance: ONE_STEP_FACTOR times the largest pose change the perturbations above
# cause over the one_step cases.  It is measured where it is used (milliseconds on the oracle)
# and has to come out at or below ONE_STEP_CEILING, four orders under the whole-solve bar of 1e-6.
ONE_STEP_FACTOR = 1000.0
ONE_STEP_CEILING = 1e-10


@functools.lru_cache(maxsize=None)
def one_step_tolerance(orc, synth):
    spread = max(one_step_spread(orc, synth))
    tolerance = ONE_STEP_FACTOR * spread
    assert 0.0 < tolerance <= ONE_STEP_CEILING, (spread, tolerance)
    return tolerance


@functools.lru_cache(maxsize=None)
def one_step_spread(orc, synth):
    """(largest |pose - unperturbed pose| over the 2D one_step cases, the same over 3D)."""
    spread2 = spread3 = 0.0
    for case in cases_2d(synth):
        if case.family == "one_step":
            base = oracle_2d(orc, synth, case)["pose"]
            spread2 = max([spread2] + [float(np.abs(r["pose"] - base).max())
                                       for r in perturbed_2d(orc, synth, case)])
    for case in cases_3d(synth, orc):
        if case.family == "one_step":
            base = oracle_3d(orc, case)["pose"]
            spread3 = max([spread3] + [float(np.abs(r["pose"] - base).max())
                                       for r in perturbed_3d(orc, case)])
    return spread2, spread3
