"""Host-side mirror of the reference's scan-matcher classes over the C ABI.

Same names, argument meaning and failure behaviour as
``cartographer/mapping/internal/2d/scan_matching/real_time_correlative_scan_matcher_2d.h:48-83``
and ``.../fast_correlative_scan_matcher_2d.h:109-160`` (3D twins in
``.../3d/scan_matching``), so the parity tests read like the reference's own
tests.  All arithmetic happens in ``libcartographer_mi355x.so``.
"""
import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib
from ._lib import (Ceres2DOptions, CeresSummary, Fast2DOptions, Grid2DLimits, MatchStats, Pose2d,
                   RtOptions, check)

K_MIN_CORRESPONDENCE_COST = float(np.float32(1) - (np.float32(1) - np.float32(0.1)))
K_MAX_CORRESPONDENCE_COST = float(np.float32(1) - np.float32(0.1))


@dataclass
class Rigid2d:
    """transform::Rigid2d: translation + rotation angle."""
    x: float = 0.0
    y: float = 0.0
    theta: float = 0.0

    def to_c(self):
        return Pose2d(self.x, self.y, self.theta)


class Grid2D:
    """Read-only view of a ProbabilityGrid: MapLimits + correspondence-cost cells."""

    def __init__(self, cells, resolution, max_x, max_y,
                 min_correspondence_cost=K_MIN_CORRESPONDENCE_COST,
                 max_correspondence_cost=K_MAX_CORRESPONDENCE_COST):
        self.cells = np.ascontiguousarray(cells, dtype=np.uint16)
        if self.cells.ndim != 2:
            raise ValueError("cells must be [num_y_cells, num_x_cells]")
        self.resolution = float(resolution)
        self.max_x = float(max_x)
        self.max_y = float(max_y)
        self.min_correspondence_cost = float(min_correspondence_cost)
        self.max_correspondence_cost = float(max_correspondence_cost)

    @property
    def num_x_cells(self):
        return self.cells.shape[1]

    @property
    def num_y_cells(self):
        return self.cells.shape[0]

    def limits_c(self):
        return Grid2DLimits(self.resolution, self.max_x, self.max_y, self.num_x_cells,
                            self.num_y_cells, self.min_correspondence_cost,
                            self.max_correspondence_cost)


class TSDF2D:
    """Read-only view of a TSDF2D (mapping/internal/2d/tsdf_2d.h): MapLimits, the tsd and
    weight planes (uint16, 0 = unknown) and the TSDValueConverter ranges."""

    def __init__(self, tsd_cells, weight_cells, resolution, max_x, max_y, truncation_distance,
                 max_weight):
        self.cells = np.ascontiguousarray(tsd_cells, dtype=np.uint16)
        self.weight_cells = np.ascontiguousarray(weight_cells, dtype=np.uint16)
        if self.cells.ndim != 2 or self.cells.shape != self.weight_cells.shape:
            raise ValueError("tsd / weight cells must both be [num_y_cells, num_x_cells]")
        self.resolution = float(resolution)
        self.max_x = float(max_x)
        self.max_y = float(max_y)
        self.truncation_distance = float(truncation_distance)
        self.max_weight = float(max_weight)

    def limits_c(self):
        # Grid2D(limits, -truncation_distance, truncation_distance) (tsdf_2d.cc:25-26)
        return Grid2DLimits(self.resolution, self.max_x, self.max_y, self.cells.shape[1],
                            self.cells.shape[0], -self.truncation_distance,
                            self.truncation_distance)


def _cloud(point_cloud):
    xyz = np.ascontiguousarray(point_cloud, dtype=np.float32).reshape(-1, 3)
    return xyz, xyz.shape[0]


class RealTimeCorrelativeScanMatcher2D:
    """RealTimeCorrelativeScanMatcher2D(options).Match(initial, cloud, grid) -> (score, pose)."""

    def __init__(self, linear_search_window, angular_search_window,
                 translation_delta_cost_weight, rotation_delta_cost_weight, device=0):
        self.options = RtOptions(linear_search_window, angular_search_window,
                                 translation_delta_cost_weight, rotation_delta_cost_weight)
        self.device = device
        self.last_stats = None

    def match(self, initial_pose_estimate, point_cloud, grid):
        xyz, n = _cloud(point_cloud)
        from .grid_2d import ProbabilityGridOnDevice, TSDF2DOnDevice
        if isinstance(grid, TSDF2DOnDevice):              # TSDF planes already in HBM
            init = initial_pose_estimate.to_c()
            score, pose, stats = C.c_double(), Pose2d(), MatchStats()
            check(_lib.lib().cmx_rt2d_match_tsdf_grid(C.byref(self.options), grid._h,
                                                      C.byref(init), xyz.ctypes.data, n,
                                                      C.byref(score), C.byref(pose),
                                                      C.byref(stats)))
            self.last_stats = stats.as_dict()
            return score.value, Rigid2d(pose.x, pose.y, pose.theta)
        if isinstance(grid, ProbabilityGridOnDevice):     # grid already in HBM
            init = initial_pose_estimate.to_c()
            score, pose, stats = C.c_double(), Pose2d(), MatchStats()
            check(_lib.lib().cmx_rt2d_match_grid(C.byref(self.options), grid._h, C.byref(init),
                                                 xyz.ctypes.data, n, C.byref(score),
                                                 C.byref(pose), C.byref(stats)))
            self.last_stats = stats.as_dict()
            return score.value, Rigid2d(pose.x, pose.y, pose.theta)
        limits = grid.limits_c()
        init = initial_pose_estimate.to_c()
        score = C.c_double()
        pose = Pose2d()
        stats = MatchStats()
        if isinstance(grid, TSDF2D):      # GridType::TSDF branch (.cc:159-167)
            check(_lib.lib().cmx_rt2d_match_tsdf(
                C.byref(self.options), C.byref(limits), grid.cells.ctypes.data,
                grid.weight_cells.ctypes.data, grid.truncation_distance, grid.max_weight,
                C.byref(init), xyz.ctypes.data, n, self.device, C.byref(score), C.byref(pose),
                C.byref(stats)))
        else:
            check(_lib.lib().cmx_rt2d_match(C.byref(self.options), C.byref(limits),
                                            grid.cells.ctypes.data, C.byref(init),
                                            xyz.ctypes.data, n, self.device, C.byref(score),
                                            C.byref(pose), C.byref(stats)))
        self.last_stats = stats.as_dict()
        return score.value, Rigid2d(pose.x, pose.y, pose.theta)


def _batch_entries(grids):
    """(host-cloud entry, resident-cloud entry) for a batch on `grids`: all ProbabilityGridOnDevice
    or all TSDF2DOnDevice; a list mixing the two classes raises."""
    from .grid_2d import TSDF2DOnDevice
    tsdf = [isinstance(g, TSDF2DOnDevice) for g in grids]
    if any(tsdf) and not all(tsdf):
        raise ValueError("a batch takes grids of one type: ProbabilityGridOnDevice or "
                         "TSDF2DOnDevice, not both")
    L = _lib.lib()
    if any(tsdf):
        return L.cmx_rt2d_match_tsdf_grid_batch, L.cmx_rt2d_match_tsdf_grid_batch_resident
    return L.cmx_rt2d_match_grid_batch, L.cmx_rt2d_match_grid_batch_resident


def rt2d_match_batch(options, grids, initial_pose_estimates, point_clouds):
    """cmx_rt2d_match_grid_batch / cmx_rt2d_match_tsdf_grid_batch: match i = (point_clouds[i],
    grids[i], initial_pose_estimates[i]); `grids` are all ProbabilityGridOnDevice or all
    TSDF2DOnDevice, `options` an RtOptions (or a RealTimeCorrelativeScanMatcher2D).  Returns
    (scores, poses, stats)."""
    if isinstance(options, RealTimeCorrelativeScanMatcher2D):
        options = options.options
    num = len(grids)
    entry = _batch_entries(grids)[0]
    clouds = [_cloud(c)[0] for c in point_clouds]
    handles = (C.c_void_p * num)(*[g._h for g in grids])
    cloud_ptrs = (C.c_void_p * num)(*[c.ctypes.data for c in clouds])
    counts = np.array([c.shape[0] for c in clouds], np.int32)
    initial = (Pose2d * num)(*[p.to_c() for p in initial_pose_estimates])
    scores = np.zeros(num, np.float64)
    poses = (Pose2d * num)()
    stats = MatchStats()
    check(entry(
        C.byref(options), handles, num, C.cast(initial, C.c_void_p), cloud_ptrs,
        counts.ctypes.data, scores.ctypes.data, C.cast(poses, C.c_void_p), C.byref(stats)))
    return (scores, [Rigid2d(p.x, p.y, p.theta) for p in poses], stats.as_dict())


class Rt2DBatch:
    """The argument arrays of cmx_rt2d_match_grid_batch (cmx_rt2d_match_tsdf_grid_batch when the
    grids are TSDF2DOnDevice), built once: what a C++ caller holds
    anyway (one resident grid and one scan buffer per trajectory / robot).  `match(poses)` takes
    the initial pose estimates as an (n, 3) float64 array (x, y, theta) and returns
    (scores, poses as an (n, 3) array, stats)."""

    def __init__(self, options, grids, point_clouds, resident=False):
        """resident=True: the scans are uploaded once (cmx_cloud) and every match() goes through
        the `_resident` entry; `point_clouds` may then also be PointCloudOnDevice."""
        if isinstance(options, RealTimeCorrelativeScanMatcher2D):
            options = options.options
        host_entry, resident_entry = _batch_entries(grids)
        self.options = options
        self.num = len(grids)
        self._grids = list(grids)                                  # keep the handles alive
        self._handles = (C.c_void_p * self.num)(*[g._h for g in grids])
        self._scores = np.zeros(self.num, np.float64)
        self._poses = np.zeros((self.num, 3), np.float64)          # cmx_pose2d[num]
        self._stats = MatchStats()
        self.resident = resident
        if resident:
            self._clouds = [c if isinstance(c, PointCloudOnDevice) else PointCloudOnDevice(c)
                            for c in point_clouds]
            self._cloud_ptrs = (C.c_void_p * self.num)(*[c._h for c in self._clouds])
            self._fn = resident_entry
        else:
            self._clouds = [_cloud(c)[0] for c in point_clouds]
            self._cloud_ptrs = (C.c_void_p * self.num)(*[c.ctypes.data for c in self._clouds])
            self._counts = np.array([c.shape[0] for c in self._clouds], np.int32)
            self._fn = host_entry

    def match(self, initial_pose_estimates):
        init = np.ascontiguousarray(initial_pose_estimates, np.float64).reshape(self.num, 3)
        if self.resident:
            check(self._fn(C.byref(self.options), self._handles, self.num, init.ctypes.data,
                           self._cloud_ptrs, self._scores.ctypes.data, self._poses.ctypes.data,
                           C.byref(self._stats)))
        else:
            check(self._fn(C.byref(self.options), self._handles, self.num, init.ctypes.data,
                           self._cloud_ptrs, self._counts.ctypes.data, self._scores.ctypes.data,
                           self._poses.ctypes.data, C.byref(self._stats)))
        return self._scores, self._poses, self._stats.as_dict()


class PointCloudOnDevice:
    """A point cloud uploaded once (cmx_cloud) for repeated resident matches."""

    def __init__(self, point_cloud, device=0):
        xyz, n = _cloud(point_cloud)
        self.num_points = n
        self._h = C.c_void_p()
        check(_lib.lib().cmx_cloud_upload(xyz.ctypes.data, n, device, C.byref(self._h)))

    def __del__(self):
        if getattr(self, "_h", None):
            _lib.lib().cmx_cloud_destroy(self._h)
            self._h = None


class FastCorrelativeScanMatcher2D:
    """FastCorrelativeScanMatcher2D(grid, options): Match / MatchFullSubmap.

    ``match*`` return ``(found, score, pose)``; ``found`` False mirrors the
    reference returning ``false`` (score/pose are then None).
    """

    def __init__(self, grid, branch_and_bound_depth, linear_search_window=7.0,
                 angular_search_window=float(np.deg2rad(30.0)), device=0):
        self.grid = grid
        self.options = Fast2DOptions(linear_search_window, angular_search_window,
                                     branch_and_bound_depth)
        self.device = device
        self.last_stats = None
        self._h = C.c_void_p()
        limits = grid.limits_c()
        check(_lib.lib().cmx_fast2d_create(C.byref(self.options), C.byref(limits),
                                           grid.cells.ctypes.data, device, C.byref(self._h)))

    @classmethod
    def from_device_grid(cls, device_grid, branch_and_bound_depth, linear_search_window=7.0,
                         angular_search_window=float(np.deg2rad(30.0))):
        """Matcher of a grid that lives in HBM (cartographer_amd.grid_2d.ProbabilityGridOnDevice,
        or TSDF2DOnDevice: the tsd plane over the cost range [-truncation, truncation])."""
        from .grid_2d import TSDF2DOnDevice
        self = cls.__new__(cls)
        self.grid = device_grid
        self.options = Fast2DOptions(linear_search_window, angular_search_window,
                                     branch_and_bound_depth)
        self.device = device_grid.device
        self.last_stats = None
        self._h = C.c_void_p()
        create = (_lib.lib().cmx_fast2d_create_from_tsdf if isinstance(device_grid, TSDF2DOnDevice)
                  else _lib.lib().cmx_fast2d_create_from_grid)
        check(create(C.byref(self.options), device_grid._h, C.byref(self._h)))
        return self

    @classmethod
    def create_batch(cls, grids, branch_and_bound_depth, linear_search_window=7.0,
                     angular_search_window=float(np.deg2rad(30.0)), device=0):
        """cmx_fast2d_create_batch: the matchers of many submaps in one call (a loaded map, the
        first global constraint of a node against every finished submap).  `grids` mixes Grid2D
        (host cells), ProbabilityGridOnDevice and TSDF2DOnDevice (resident on `device`); returns
        ordinary matcher objects, each what the constructor / from_device_grid builds."""
        from .grid_2d import ProbabilityGridOnDevice, TSDF2DOnDevice
        grids = list(grids)
        num = len(grids)
        options = Fast2DOptions(linear_search_window, angular_search_window,
                                branch_and_bound_depth)
        sources = (_lib.Fast2DSource * max(num, 1))()
        keep = []                                   # limits and cell arrays the sources point at
        for k, grid in enumerate(grids):
            if isinstance(grid, TSDF2DOnDevice):
                sources[k].tsdf = grid._h
            elif isinstance(grid, ProbabilityGridOnDevice):
                sources[k].grid = grid._h
            else:
                limits = grid.limits_c()
                cells = np.ascontiguousarray(grid.cells, np.uint16)
                keep.append((limits, cells))
                sources[k].limits = C.pointer(limits)
                sources[k].cells = cells.ctypes.data
        handles = (C.c_void_p * max(num, 1))()
        check(_lib.lib().cmx_fast2d_create_batch(C.byref(options), sources, num, device, handles))
        del keep
        matchers = []
        for k, grid in enumerate(grids):
            self = cls.__new__(cls)
            self.grid = grid
            self.options = Fast2DOptions(linear_search_window, angular_search_window,
                                         branch_and_bound_depth)
            self.device = device
            self.last_stats = None
            self._h = C.c_void_p(handles[k])
            matchers.append(self)
        return matchers

    def __del__(self):
        if getattr(self, "_h", None):
            _lib.lib().cmx_fast2d_destroy(self._h)
            self._h = None

    def _result(self, found, score, pose, stats):
        self.last_stats = stats.as_dict()
        if not found.value:
            return False, None, None
        return True, float(score.value), Rigid2d(pose.x, pose.y, pose.theta)

    def match(self, initial_pose_estimate, point_cloud, min_score):
        xyz, n = _cloud(point_cloud)
        init = initial_pose_estimate.to_c()
        found, score, pose, stats = C.c_int32(), C.c_float(), Pose2d(), MatchStats()
        check(_lib.lib().cmx_fast2d_match(self._h, C.byref(init), xyz.ctypes.data, n, min_score,
                                          C.byref(found), C.byref(score), C.byref(pose),
                                          C.byref(stats)))
        return self._result(found, score, pose, stats)

    def match_full_submap(self, point_cloud, min_score):
        xyz, n = _cloud(point_cloud)
        found, score, pose, stats = C.c_int32(), C.c_float(), Pose2d(), MatchStats()
        check(_lib.lib().cmx_fast2d_match_full_submap(self._h, xyz.ctypes.data, n, min_score,
                                                      C.byref(found), C.byref(score),
                                                      C.byref(pose), C.byref(stats)))
        return self._result(found, score, pose, stats)

    # -- introspection for the parity tests ---------------------------------
    def level(self, i):
        wx, wy = C.c_int32(), C.c_int32()
        check(_lib.lib().cmx_fast2d_level_dims(self._h, i, C.byref(wx), C.byref(wy)))
        out = np.empty((wy.value, wx.value), np.uint8)
        check(_lib.lib().cmx_fast2d_level_cells(self._h, i, out.ctypes.data))
        return out

    def debug_prepare(self, initial_pose_estimate, point_cloud, full_submap):
        xyz, n = _cloud(point_cloud)
        init = (initial_pose_estimate or Rigid2d()).to_c()
        ns, step, ncoarse = C.c_int32(), C.c_double(), C.c_int64()
        L = _lib.lib()
        check(L.cmx_fast2d_debug_prepare(self._h, C.byref(init), xyz.ctypes.data, n,
                                         int(full_submap), C.byref(ns), C.byref(step), None, 0,
                                         None, 0, None, 0, C.byref(ncoarse)))
        scans = np.empty((ns.value, n, 2), np.int32)
        bounds = np.empty((ns.value, 4), np.int32)
        sums = np.empty(ncoarse.value, np.int32)
        check(L.cmx_fast2d_debug_prepare(self._h, C.byref(init), xyz.ctypes.data, n,
                                         int(full_submap), C.byref(ns), C.byref(step),
                                         scans.ctypes.data, scans.size, bounds.ctypes.data,
                                         bounds.size, sums.ctypes.data, sums.size,
                                         C.byref(ncoarse)))
        return dict(num_scans=ns.value, step=step.value, scans=scans, bounds=bounds, sums=sums)


def debug_plan(matchers, match_full_submap, point_cloud=None, num_points=None, max_range_xy=None):
    """cmx_debug_fast2d_plan: the routes the fast 2D front end would give the problems of one
    call and the sizes of its launches; nothing is launched.  `matchers` are
    FastCorrelativeScanMatcher2D objects, or -- no device needed -- (Grid2DLimits, Fast2DOptions)
    pairs of the matchers one would create; `match_full_submap` as in match_batch (None: all
    windowed).  The cloud enters through its size and its largest xy range: pass it, or the two
    numbers.  Returns (problems, launch): a list of dicts (use_planes, plane_stride, use_fused,
    group, acc, num_scans) and a dict (fused_lds, fused_acc, any_group, plane_acc_cells,
    max_scans, per_unit)."""
    num = len(matchers)
    if point_cloud is not None:
        xyz, num_points = _cloud(point_cloud)
        x, y = xyz[:, 0], xyz[:, 1]
        max_range_xy = float(np.sqrt(x * x + y * y).max()) if num_points else 0.0   # f32, as the library
    handles = limits = options = None
    if all(isinstance(m, FastCorrelativeScanMatcher2D) for m in matchers):
        handles = (C.c_void_p * num)(*[m._h for m in matchers])
    else:
        limits = (Grid2DLimits * num)(*[m[0] for m in matchers])
        options = (Fast2DOptions * num)(*[m[1] for m in matchers])
    full = None if match_full_submap is None else np.ascontiguousarray(match_full_submap, np.int32)
    problems = (_lib.DebugFast2DProblemPlan * num)()
    launch = _lib.DebugFast2DLaunchPlan()
    check(_lib.lib().cmx_debug_fast2d_plan(
        handles, limits, options, num, None if full is None else full.ctypes.data,
        int(num_points), float(max_range_xy), problems, C.byref(launch)))

    def as_dict(s_):
        return {name: int(getattr(s_, name)) for name, _ in s_._fields_ if name != "reserved"}
    return [as_dict(p) for p in problems], as_dict(launch)


def match_full_submap_batch(matchers, point_cloud, min_score):
    """One scan against many submaps: the ConstraintBuilder2D fan-out
    (constraints/constraint_builder_2d.cc:97-137) as a single device batch.

    ``point_cloud`` is an array or a PointCloudOnDevice.  Returns
    (found[int32], scores[float32], poses[n,3], stats dict).
    """
    num = len(matchers)
    handles = (C.c_void_p * num)(*[m._h for m in matchers])
    found = np.zeros(num, np.int32)
    scores = np.zeros(num, np.float32)
    poses = np.zeros((num, 3), np.float64)
    stats = MatchStats()
    L = _lib.lib()
    if isinstance(point_cloud, PointCloudOnDevice):
        check(L.cmx_fast2d_match_full_submap_batch_resident(
            handles, num, point_cloud._h, min_score, found.ctypes.data, scores.ctypes.data,
            poses.ctypes.data, C.byref(stats)))
    else:
        xyz, n = _cloud(point_cloud)
        check(L.cmx_fast2d_match_full_submap_batch(handles, num, xyz.ctypes.data, n, min_score,
                                                   found.ctypes.data, scores.ctypes.data,
                                                   poses.ctypes.data, C.byref(stats)))
    return found, scores, poses, stats.as_dict()


def match_batch(matchers, initial_pose_estimates, match_full_submap, min_scores, point_cloud):
    """cmx_fast2d_match_batch: one node's scan against many submaps, entry i either a windowed
    Match around initial_pose_estimates[i] (match_full_submap[i] == 0, MaybeAddConstraint) or a
    MatchFullSubmap (!= 0, MaybeAddGlobalConstraint), each against its own threshold
    (constraints/constraint_builder_2d.cc:77-137, :194-236).  Returns
    (found[int32], scores[float32], poses[list of Rigid2d], stats dict)."""
    num = len(matchers)
    handles = (C.c_void_p * num)(*[m._h for m in matchers])
    initial = (Pose2d * num)(*[p.to_c() for p in initial_pose_estimates])
    full = np.ascontiguousarray(match_full_submap, np.int32)
    thresholds = np.ascontiguousarray(min_scores, np.float32)
    xyz, n = _cloud(point_cloud)
    found = np.zeros(num, np.int32)
    scores = np.zeros(num, np.float32)
    poses = (Pose2d * num)()
    stats = MatchStats()
    check(_lib.lib().cmx_fast2d_match_batch(
        handles, num, C.cast(initial, C.c_void_p), full.ctypes.data, thresholds.ctypes.data,
        xyz.ctypes.data, n, found.ctypes.data, scores.ctypes.data, C.cast(poses, C.c_void_p),
        C.byref(stats)))
    return found, scores, [Rigid2d(p.x, p.y, p.theta) for p in poses], stats.as_dict()


def _pair_clouds(point_clouds):
    """The clouds of a list of pairs as (resident, pointer array, counts, keep-alive list): all
    arrays or all PointCloudOnDevice; an object that repeats in the list (one node in several
    pairs) becomes a repeated pointer, so that the library sees one node."""
    num = len(point_clouds)
    resident = [isinstance(c, PointCloudOnDevice) for c in point_clouds]
    if any(resident) and not all(resident):
        raise ValueError("the clouds of a call are all arrays or all PointCloudOnDevice")
    if num and all(resident):
        pointers = (C.c_void_p * num)(*[c._h for c in point_clouds])
        return True, pointers, None, list(point_clouds)
    converted = {}
    for c in point_clouds:
        if id(c) not in converted:
            converted[id(c)] = _cloud(c)[0]
    arrays = [converted[id(c)] for c in point_clouds]
    pointers = (C.c_void_p * num)(*[a.ctypes.data if a.shape[0] else None for a in arrays])
    counts = np.array([a.shape[0] for a in arrays], np.int32)
    return False, pointers, counts, arrays


def match_pairs(matchers, initial_pose_estimates, match_full_submap, min_scores, point_clouds):
    """cmx_fast2d_match_pairs[_resident]: a list of (node, submap) pairs, pair p its own cloud
    point_clouds[p] against matchers[p] -- the burst of PoseGraph2D::ComputeConstraintsForNode
    when a submap finishes (pose_graph_2d.cc:383-393), or any other list.  Entries as in
    match_batch; `point_clouds` are arrays or PointCloudOnDevice (one kind per call), and an object
    named by several pairs is one node.  `initial_pose_estimates` may be None when every pair is a
    full-submap search.  Returns (found[int32], scores[float32], poses[list of Rigid2d],
    stats dict); every pair's result is what the single call returns for it."""
    num = len(matchers)
    handles = (C.c_void_p * num)(*[m._h for m in matchers])
    initial = None
    if initial_pose_estimates is not None:
        initial = (Pose2d * num)(*[p.to_c() for p in initial_pose_estimates])
    full = np.ascontiguousarray(match_full_submap, np.int32)
    thresholds = np.ascontiguousarray(min_scores, np.float32)
    resident, pointers, counts, keep = _pair_clouds(point_clouds)
    found = np.zeros(num, np.int32)
    scores = np.zeros(num, np.float32)
    poses = (Pose2d * num)()
    stats = MatchStats()
    L = _lib.lib()
    head = (handles, num, None if initial is None else C.cast(initial, C.c_void_p),
            full.ctypes.data, thresholds.ctypes.data, pointers)
    tail = (found.ctypes.data, scores.ctypes.data, C.cast(poses, C.c_void_p), C.byref(stats))
    if resident:
        check(L.cmx_fast2d_match_pairs_resident(*head, *tail))
    else:
        check(L.cmx_fast2d_match_pairs(*head, counts.ctypes.data, *tail))
    del keep
    return found, scores, [Rigid2d(p.x, p.y, p.theta) for p in poses], stats.as_dict()


class CeresScanMatcher2D:
    """CeresScanMatcher2D(options).Match(target_translation, initial_pose_estimate, point_cloud,
    grid) -> (pose_estimate, summary)  (ceres_scan_matcher_2d.h:44-56).  `grid` is a Grid2D or a
    grid resident in HBM (cartographer_amd.grid_2d.ProbabilityGridOnDevice), refined with the
    occupied-space cost, or a TSDF2D / TSDF2DOnDevice, refined with TSDFMatchCostFunction2D
    (the GridType::TSDF case, ceres_scan_matcher_2d.cc:83-90)."""

    def __init__(self, occupied_space_weight, translation_weight, rotation_weight,
                 use_nonmonotonic_steps=False, max_num_iterations=20, device=0):
        self.options = Ceres2DOptions(occupied_space_weight, translation_weight, rotation_weight,
                                      1 if use_nonmonotonic_steps else 0, max_num_iterations)
        self.device = device

    def match(self, target_translation, initial_pose_estimate, point_cloud, grid):
        from .grid_2d import ProbabilityGridOnDevice, TSDF2DOnDevice
        xyz, n = _cloud(point_cloud)
        target = np.ascontiguousarray(target_translation, np.float64)
        init = initial_pose_estimate.to_c()
        pose, summary = Pose2d(), CeresSummary()
        cloud = xyz.ctypes.data if n else None
        if isinstance(grid, TSDF2DOnDevice):
            check(_lib.lib().cmx_ceres2d_match_tsdf_grid(C.byref(self.options), grid._h,
                                                         target.ctypes.data, C.byref(init),
                                                         cloud, n, C.byref(pose),
                                                         C.byref(summary)))
        elif isinstance(grid, TSDF2D):
            limits = grid.limits_c()
            check(_lib.lib().cmx_ceres2d_match_tsdf(
                C.byref(self.options), C.byref(limits), grid.cells.ctypes.data,
                grid.weight_cells.ctypes.data, grid.truncation_distance, grid.max_weight,
                target.ctypes.data, C.byref(init), cloud, n, self.device, C.byref(pose),
                C.byref(summary)))
        elif isinstance(grid, ProbabilityGridOnDevice):
            check(_lib.lib().cmx_ceres2d_match_grid(C.byref(self.options), grid._h,
                                                    target.ctypes.data, C.byref(init),
                                                    xyz.ctypes.data, n, C.byref(pose),
                                                    C.byref(summary)))
        else:
            limits = grid.limits_c()
            check(_lib.lib().cmx_ceres2d_match(C.byref(self.options), C.byref(limits),
                                               grid.cells.ctypes.data, target.ctypes.data,
                                               C.byref(init), xyz.ctypes.data, n, self.device,
                                               C.byref(pose), C.byref(summary)))
        return Rigid2d(pose.x, pose.y, pose.theta), summary.as_dict()

    def refine_batch(self, matchers, found, pose_estimates, point_cloud):
        """ConstraintBuilder2D::ComputeConstraint's refinement of a batch of search results
        (constraint_builder_2d.cc:245-249), each against the grid its matcher keeps in HBM."""
        num = len(matchers)
        xyz, n = _cloud(point_cloud)
        handles = (C.c_void_p * num)(*[m._h for m in matchers])
        found = np.ascontiguousarray(found, np.int32)
        poses_in = (Pose2d * num)(*[p.to_c() for p in pose_estimates])
        poses_out = (Pose2d * num)()
        summaries = (CeresSummary * num)()
        check(_lib.lib().cmx_fast2d_refine_batch(
            C.byref(self.options), handles, num, found.ctypes.data, C.cast(poses_in, C.c_void_p),
            xyz.ctypes.data, n, C.cast(poses_out, C.c_void_p), C.cast(summaries, C.c_void_p)))
        return ([Rigid2d(p.x, p.y, p.theta) for p in poses_out],
                [s_.as_dict() for s_ in summaries])

    def refine_batch_tsdf(self, grids, found, pose_estimates, point_cloud):
        """The same refinement against finished TSDF submaps kept in HBM (TSDF2DOnDevice): entry
        i refines pose_estimates[i] towards its own translation; found[i] == 0 passes through.
        One launch per device the grids live on."""
        num = len(grids)
        xyz, n = _cloud(point_cloud)
        handles = (C.c_void_p * num)(*[g._h for g in grids])
        found = None if found is None else np.ascontiguousarray(found, np.int32)
        poses_in = (Pose2d * num)(*[p.to_c() for p in pose_estimates])
        poses_out = (Pose2d * num)()
        summaries = (CeresSummary * num)()
        check(_lib.lib().cmx_ceres2d_refine_batch_tsdf(
            C.byref(self.options), handles, num, None if found is None else found.ctypes.data,
            C.cast(poses_in, C.c_void_p), xyz.ctypes.data if n else None, n,
            C.cast(poses_out, C.c_void_p), C.cast(summaries, C.c_void_p)))
        return ([Rigid2d(p.x, p.y, p.theta) for p in poses_out],
                [s_.as_dict() for s_ in summaries])


    def _refine_pairs(self, entry, resident_entry, handles_of, found, pose_estimates,
                      point_clouds):
        num = len(handles_of)
        handles = (C.c_void_p * num)(*[h._h for h in handles_of])
        found = None if found is None else np.ascontiguousarray(found, np.int32)
        poses_in = (Pose2d * num)(*[p.to_c() for p in pose_estimates])
        poses_out = (Pose2d * num)()
        summaries = (CeresSummary * num)()
        resident, pointers, counts, keep = _pair_clouds(point_clouds)
        head = (C.byref(self.options), handles, num, None if found is None else found.ctypes.data,
                C.cast(poses_in, C.c_void_p), pointers)
        tail = (C.cast(poses_out, C.c_void_p), C.cast(summaries, C.c_void_p))
        if resident:
            if resident_entry is None:
                raise ValueError("this refinement takes host clouds")
            check(resident_entry(*head, *tail))
        else:
            check(entry(*head, counts.ctypes.data, *tail))
        del keep
        return ([Rigid2d(p.x, p.y, p.theta) for p in poses_out],
                [s_.as_dict() for s_ in summaries])

    def refine_pairs(self, matchers, found, pose_estimates, point_clouds):
        """cmx_fast2d_refine_pairs[_resident]: refine_batch for the results of match_pairs, pair
        p with its own cloud point_clouds[p] (arrays or PointCloudOnDevice, one kind per call;
        an object named by several pairs is staged once), in ONE launch for the whole list.
        found[p] == 0 passes through; found=None refines every pair."""
        L = _lib.lib()
        return self._refine_pairs(L.cmx_fast2d_refine_pairs, L.cmx_fast2d_refine_pairs_resident,
                                  matchers, found, pose_estimates, point_clouds)

    def refine_pairs_tsdf(self, grids, found, pose_estimates, point_clouds):
        """cmx_ceres2d_refine_pairs_tsdf: the same against finished TSDF submaps kept in HBM
        (TSDF2DOnDevice), pair p with its own host cloud; an empty cloud ends with FAILURE and
        the pose untouched, as in refine_batch_tsdf."""
        return self._refine_pairs(_lib.lib().cmx_ceres2d_refine_pairs_tsdf, None, grids, found,
                                  pose_estimates, point_clouds)

    def match_batch(self, target_translations, initial_pose_estimates, point_clouds, grids):
        """cmx_ceres2d_match_grid_batch: `match` for many robots in one call, one upload, one
        launch and one synchronisation -- the Ceres match of LocalTrajectoryBuilder2D::ScanMatch
        for a fleet.  Job i matches point_clouds[i] (an array or a PointCloudOnDevice; the same
        array object listed twice is one cloud, staged once) against grids[i] (a
        ProbabilityGridOnDevice or a TSDF2DOnDevice, in any mixture; a grid may repeat) from
        initial_pose_estimates[i] towards target_translations[i].  Returns (poses, summaries),
        per job what `match` returns for it, bit for bit."""
        from .grid_2d import ProbabilityGridOnDevice, TSDF2DOnDevice
        num = len(grids)
        if not (len(target_translations) == len(initial_pose_estimates) == len(point_clouds)
                == num):
            raise ValueError("one target, initial pose, cloud and grid per job")
        jobs = (_lib.Ceres2DJob * max(num, 1))()
        converted = {}
        for i, (target, initial, cloud, grid) in enumerate(
                zip(target_translations, initial_pose_estimates, point_clouds, grids)):
            job = jobs[i]
            if isinstance(grid, TSDF2DOnDevice):
                job.tsdf = grid._h
            elif isinstance(grid, ProbabilityGridOnDevice):
                job.grid = grid._h
            else:
                raise TypeError(f"job {i}: the grid is neither a ProbabilityGridOnDevice nor a "
                                "TSDF2DOnDevice")
            if isinstance(cloud, PointCloudOnDevice):
                job.cloud = cloud._h
            else:
                if id(cloud) not in converted:
                    converted[id(cloud)] = _cloud(cloud)[0]
                xyz = converted[id(cloud)]
                job.point_cloud_xyz = xyz.ctypes.data if xyz.shape[0] else None
                job.num_points = xyz.shape[0]
            target = np.asarray(target, np.float64).reshape(2)
            job.target_translation_xy[0], job.target_translation_xy[1] = target[0], target[1]
            job.initial_pose_estimate = initial.to_c()
        poses = (Pose2d * max(num, 1))()
        summaries = (CeresSummary * max(num, 1))()
        check(_lib.lib().cmx_ceres2d_match_grid_batch(C.byref(self.options), jobs, num,
                                                      C.cast(poses, C.c_void_p),
                                                      C.cast(summaries, C.c_void_p)))
        del converted
        return ([Rigid2d(p.x, p.y, p.theta) for p in poses[:num]],
                [s_.as_dict() for s_ in summaries[:num]])


def ceres2d_batch_plan(kinds, point_clouds_or_counts, resident=None):
    """cmx_debug_ceres2d_batch_plan: the plan of a CeresScanMatcher2D.match_batch call -- the
    layout of its one upload block and its number of launches -- without a grid or a device.
    kinds[i] is 0 (probability grid) or 1 (TSDF).  point_clouds_or_counts[i] is an array (the
    same object twice is one cloud), a PointCloudOnDevice (resident), an int (a host cloud of its
    own with that many points; 0: none), or a pair (array, count) that names the array's memory
    with another count.  `resident` (flags per job) marks int entries as resident clouds.
    Returns (jobs, call): per job {"kind", "cloud_slot", "cloud_offset"}, for the call
    {"total_bytes", "problem_bytes", "num_clouds", "num_launches"}."""
    num = len(kinds)
    kinds = np.ascontiguousarray(kinds, np.int32)
    pointers = (C.c_void_p * max(num, 1))()
    counts = np.zeros(max(num, 1), np.int32)
    flags = np.zeros(max(num, 1), np.int32)
    if resident is not None:
        flags[:num] = np.asarray(resident, np.int32)
    keep = {}
    for i, entry in enumerate(point_clouds_or_counts):
        count = None
        if isinstance(entry, tuple):
            entry, count = entry
        if isinstance(entry, PointCloudOnDevice):
            flags[i], counts[i] = 1, entry.num_points
        elif isinstance(entry, (int, np.integer)):
            counts[i] = entry
            if entry > 0 and not flags[i]:
                # an identity of its own: one float per job, never read
                keep[("own", i)] = np.zeros(1, np.float32)
                pointers[i] = keep[("own", i)].ctypes.data
        else:
            if id(entry) not in keep:
                keep[id(entry)] = _cloud(entry)[0]
            xyz = keep[id(entry)]
            counts[i] = xyz.shape[0] if count is None else count
            pointers[i] = xyz.ctypes.data if xyz.shape[0] else None
    job_plans = (_lib.DebugCeres2DJobPlan * max(num, 1))()
    call_plan = _lib.DebugCeres2DCallPlan()
    check(_lib.lib().cmx_debug_ceres2d_batch_plan(kinds.ctypes.data, pointers, counts.ctypes.data,
                                                  flags.ctypes.data, num, job_plans,
                                                  C.byref(call_plan)))
    del keep
    fields = lambda s_: {k: getattr(s_, k) for k, _ in s_._fields_}
    return [fields(p) for p in job_plans[:num]], fields(call_plan)


def tsdf_match_residuals(grid, residual_scaling_factor, pose, point_cloud, device=0):
    """TSDFMatchCostFunction2D::Evaluate (tsdf_match_cost_function_2d.cc:40-66) on a host TSDF2D
    at `pose` (x, y, theta): (valid, residuals [n], jacobian [n, 3]).  `valid` is False where the
    reference's functor returns false (every interpolated weight 0); the arrays are then None."""
    xyz, n = _cloud(point_cloud)
    limits = grid.limits_c()
    pose = np.ascontiguousarray(pose, np.float64).reshape(3)
    residuals = np.zeros(max(n, 1), np.float64)
    jacobian = np.zeros((max(n, 1), 3), np.float64)
    valid = C.c_int32()
    check(_lib.lib().cmx_ceres2d_tsdf_residuals(
        C.byref(limits), grid.cells.ctypes.data, grid.weight_cells.ctypes.data,
        grid.truncation_distance, grid.max_weight, residual_scaling_factor, pose.ctypes.data,
        xyz.ctypes.data if n else None, n, device, residuals.ctypes.data, jacobian.ctypes.data,
        C.byref(valid)))
    if not valid.value:
        return False, None, None
    return True, residuals[:n].copy(), jacobian[:n].copy()
